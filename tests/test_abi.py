"""CPU-side checks of the C ABI: the library loads and exports every symbol include/*.h declares,
and the Python seam refuses CPU tensors (no silent CPU fallback)."""

import ctypes
import keyword
import re
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT


def declared_functions():
    text = "\n".join(p.read_text() for p in sorted((ROOT / "include").glob("*.h")))
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(g2048_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_boundary():
    names = declared_functions()
    for required in ("g2048_env_step", "g2048_env_reset", "g2048_legal_mask", "g2048_obs_encode",
                     "g2048_sample_actions", "g2048_reward_rtg", "g2048_rtg_prepare", "g2048_rtg_finalize",
                     "g2048_mt_seed", "g2048_obs_gather", "g2048_ln_act_fwd", "g2048_ln_act_bwd",
                     "g2048_ppo_head_loss", "g2048_ppo_head_kl"):
        assert required in names


def test_library_exports_every_declared_symbol():
    from g2048 import _lib
    lib = _lib.load()
    for name in declared_functions():
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, f"{name}: declared, but the binding did not bind it"
    bound = {n for n, f in vars(lib).items() if n.startswith("g2048_") and f.argtypes is not None}
    assert bound == set(declared_functions())
    assert b"gfx950" in lib.g2048_build_info()
    assert lib.g2048_mt_state_words() == 625


def test_library_is_gfx950_code_object():
    from g2048 import _lib
    data = _lib.LIB_PATH.read_bytes()
    assert b"gfx950" in data


def test_cpu_tensors_are_rejected():
    from g2048 import _lib
    b = torch.zeros(4, 16, dtype=torch.int8)
    f = torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(_lib.G2048Error):
        _lib.legal_mask(b, f)


def test_struct_layouts_match_header():
    from g2048 import _lib
    assert ctypes.sizeof(_lib.Rng) == 48
    assert _lib.Rng.counter_dev.offset == 24
    assert ctypes.sizeof(_lib.RewardCfg) == 40
    assert ctypes.sizeof(_lib.Dropout) == 40
    assert _lib.Dropout.counter_dev.offset == 32
    assert ctypes.sizeof(_lib.PPOBatch) == 56 and _lib.PPOBatch.rows.offset == 48
    assert ctypes.sizeof(_lib.Dy) == 64 and _lib.Dy.dz.offset == 40 and _lib.DY_MAX_P == 4
    assert ctypes.sizeof(_lib.ColsumJob) == 88 and _lib.ColsumJob.len.offset == 64
    assert ctypes.sizeof(_lib.MlpPassArgs) == 424 and _lib.MlpPassArgs.drop.offset == 176
    assert _lib.MlpPassArgs.keep.offset == 408 and _lib.MlpPassArgs.idx_offset.offset == 416
    assert ctypes.sizeof(_lib.PPOStatsArgs) == 88 and _lib.PPOStatsArgs.idx_offset.offset == 72
    assert ctypes.sizeof(_lib.MlpBackArgs) == 312 and _lib.MlpBackArgs.keep.offset == 304
    assert ctypes.sizeof(_lib.MuonCfg) == 48 and _lib.MuonCfg.workspace.offset == 40
    assert ctypes.sizeof(_lib.MuonMatrix) == 56 and _lib.MuonMatrix.head_frag.offset == 32
    assert _lib.MlpPassArgs.partials.offset == 400


def test_struct_layouts_match_the_c_compiler(tmp_path):
    """Every generated structure against the host C compiler's own sizeof / offsetof of the headers."""
    from g2048 import _lib
    headers = [ROOT / "include" / h for h in _lib.HEADERS]
    declared = re.findall(r"typedef\s+struct\s+(\w+)\s*\{", "\n".join(h.read_text() for h in headers))
    want = {}
    lines = ["#include <stddef.h>", "#include <stdio.h>"] + [f'#include "{h.name}"' for h in headers]
    lines.append("int main(void) {")
    for cname, cls in _lib._STRUCTS.items():
        want[cname] = ctypes.sizeof(cls)
        lines.append(f'    printf("{cname} %zu\\n", sizeof({cname}));')
        for pyname, _ in cls._fields_:
            field = pyname[:-1] if pyname.endswith("_") and keyword.iskeyword(pyname[:-1]) else pyname
            f = getattr(cls, pyname)
            want[f"{cname}.{field}"] = (f.offset, f.size)
            lines.append(f'    printf("{cname}.{field} %zu %zu\\n", offsetof({cname}, {field}), '
                         f'sizeof((({cname} *)0)->{field}));')
    lines += ["    return 0;", "}", ""]
    assert sorted(declared) == sorted(_lib._STRUCTS)
    assert "g2048_dropout.pass" in want and sum("." in k for k in want) == sum(
        len(c._fields_) for c in _lib._STRUCTS.values())
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([shutil.which("cc") or "gcc", "-std=c11", "-Wall", "-Wextra", "-I", str(ROOT / "include"),
                    "-o", str(exe), str(src)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        key, *nums = line.split()
        got[key] = int(nums[0]) if len(nums) == 1 else tuple(int(x) for x in nums)
    assert got == want


def test_signatures_spot_checks():
    """A few rows of the generated prototype table spelled out by hand."""
    from g2048 import _lib
    lib = _lib.load()
    vp, i64, i32, u32, u64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64
    sz, f32, f64, P = ctypes.c_size_t, ctypes.c_float, ctypes.c_double, ctypes.POINTER
    rp, jp = P(_lib.Rng), P(_lib.ColsumJob)
    expected = {
        "g2048_env_step": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, rp, u32]),
        "g2048_mc_search": (ctypes.c_int, [vp, vp, i64, i64, i64, rp, vp, vp, vp, vp, vp, sz]),
        "g2048_ppo_backward": (ctypes.c_int, [vp, P(_lib.MlpBackArgs), P(vp), P(vp), jp]),
        "g2048_muon_adamw_step_clip": (ctypes.c_int, [vp, P(_lib.MuonMatrix), i32, P(_lib.AdamWGroup), i32, vp, vp, vp,
                                                      f32, vp, vp, P(_lib.MuonCfg), f64, f64, f32, f32]),
        "g2048_urm_forward_drop": (ctypes.c_int, [vp, P(_lib.UrmWeights), vp, i32, vp, vp, i64, f32, u64, vp]),
        "g2048_reward_rtg_workspace_bytes": (sz, [i64]),
        "g2048_build_info": (ctypes.c_char_p, []),
    }
    for name, (restype, argtypes) in expected.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, name
        assert len(fn.argtypes) == len(argtypes), name
        for i, (got, want) in enumerate(zip(fn.argtypes, argtypes)):
            assert got is want, f"{name}: parameter {i} is {got}, expected {want}"


def test_parser_refuses_what_it_does_not_understand():
    from g2048 import _lib
    ok = "#define G2048_N 2\ntypedef struct g2048_dy { const float *p[G2048_N]; } g2048_dy;\n" \
         "int g2048_f(g2048_stream_t stream, const g2048_dy *dy, int64_t n);\n"
    consts, structs, protos = {}, {}, {}
    _lib._parse_header(ok, consts, structs, protos)
    assert consts == {"N": 2} and ctypes.sizeof(structs["g2048_dy"]) == 16
    assert protos["g2048_f"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(structs["g2048_dy"]), ctypes.c_int64])
    with pytest.raises(_lib.G2048Error, match="g2048_bad_param.*long double"):
        _lib._parse_header("int g2048_bad_param(g2048_stream_t stream, long double x);", {}, {}, {})
    with pytest.raises(_lib.G2048Error, match="g2048_bad_type.*wchar_t"):
        _lib._parse_header("int g2048_bad_type(g2048_stream_t stream, const wchar_t *s);", {}, {}, {})
    with pytest.raises(_lib.G2048Error, match="g2048_bad_ret"):
        _lib._parse_header("unsigned g2048_bad_ret(void);", {}, {}, {})
    with pytest.raises(_lib.G2048Error, match="g2048_rng.*short"):
        _lib._parse_header("typedef struct g2048_rng { int32_t mode; short x; } g2048_rng;", {}, {}, {})
    with pytest.raises(_lib.G2048Error, match="g2048_rng.*G2048_UNKNOWN"):
        _lib._parse_header("typedef struct g2048_rng { float *p[G2048_UNKNOWN]; } g2048_rng;", {}, {}, {})
    with pytest.raises(_lib.G2048Error, match="g2048_new_thing"):
        _lib._parse_header("typedef struct g2048_new_thing { int32_t x; } g2048_new_thing;", {}, {}, {})


def test_urm_wgrad_supported_shapes():
    """The URM training Functions pick g2048_urm_wgrad only for shapes it accepts (<= 64 output
    tiles): hidden 64 (default) qkv / o / gate_up / down yes; hidden 80 qkv (240 x 80 = 75 tiles) and
    hidden 192 o_proj (144 tiles) fall back to autocast's nn.Linear."""
    from g2048 import _lib
    for n, k in ((192, 64), (64, 64), (240, 64), (64, 120)):
        assert _lib.urm_wgrad_supported(n, k), (n, k)
    for n, k in ((240, 80), (192, 192), (256, 256), (8, 64), (64, 60)):
        assert not _lib.urm_wgrad_supported(n, k), (n, k)
