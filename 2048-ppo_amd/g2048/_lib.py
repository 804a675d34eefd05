"""ctypes binding of libg2048.so for torch tensors on a ROCm device, generated from include/*.h.

This is the Python seam of the C ABI: every function takes torch tensors that already live on the
GPU, passes their data pointers and torch's current HIP stream, and raises on a non-zero status.
There is no CPU fallback: a missing library or a CPU tensor is an error (fail loudly).

The headers are the one description of the ABI.  At import this module parses them into the
constants (`#define G2048_X` -> `X`), the `ctypes.Structure` classes (`_STRUCT_NAMES`) and the
prototype table that `load()` binds; a declaration the parser does not understand is an error.
A new entry point is declared in the header, implemented in csrc/ and wrapped below: nothing else.
"""

from __future__ import annotations

import ctypes
import keyword
import os
import re
from pathlib import Path

import torch

LIB_PATH = Path(__file__).resolve().parent / "libg2048.so"
INCLUDE_DIR = Path(__file__).resolve().parents[2] / "include"
HEADERS = ("g2048.h", "g2048_ntuple.h", "g2048_ppo.h", "g2048_urm.h")  # in this order: a nested struct is known when it is used


class G2048Error(RuntimeError):
    pass


# ------------------------------------------------------------------------ header parser ------
_STRUCT_NAMES = {
    "g2048_rng": "Rng",
    "g2048_reward_cfg": "RewardCfg",
    "g2048_ntuple_net": "NtNet",
    "g2048_ntuple_staged_net": "NtStagedNet",
    "g2048_ntuple_carousel": "NtCarousel",
    "g2048_dropout": "Dropout",
    "g2048_policy_rollout_args": "PolicyRolloutArgs",
    "g2048_colsum_job": "ColsumJob",
    "g2048_dy": "Dy",
    "g2048_ppo_batch": "PPOBatch",
    "g2048_mlp_pass_args": "MlpPassArgs",
    "g2048_ppo_stats_args": "PPOStatsArgs",
    "g2048_mlp_back_args": "MlpBackArgs",
    "g2048_mlp_wgrad_args": "MlpWgradArgs",
    "g2048_muon_matrix": "MuonMatrix",
    "g2048_muon_cfg": "MuonCfg",
    "g2048_adamw_group": "AdamWGroup",
    "g2048_urm_weights": "UrmWeights",
}
_SCALARS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
            "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float,
            "double": ctypes.c_double, "g2048_stream_t": ctypes.c_void_p}
_POINTEES = set(_SCALARS) - {"g2048_stream_t"} | {"void", "int8_t", "uint8_t", "uint16_t"}
_TYPE = r"(?:const\s+)?(?:struct\s+)?(\w+)"
_STARS = r"((?:\*\s*(?:const\b\s*)?)*)"
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", re.S)


def _ctype(base: str, stars: str, structs: dict, decl: str):
    """The ctypes type of `base` behind stars.count("*") pointers; decl is the declaration, for the error."""
    depth = stars.count("*")
    if depth == 0 and base in _SCALARS:
        return _SCALARS[base]
    if depth == 0 and base in structs:
        return structs[base]
    if depth == 1 and base in structs:
        return ctypes.POINTER(structs[base])
    if depth == 1 and base == "char":
        return ctypes.c_char_p
    if depth == 1 and base in _POINTEES:
        return ctypes.c_void_p
    if depth == 2 and base in _POINTEES:
        return ctypes.POINTER(ctypes.c_void_p)
    raise G2048Error(f"include/*.h: type `{base} {'*' * depth}` of `{decl}` has no ctypes mapping")


def _parse_header(text: str, consts: dict, structs: dict, protos: dict):
    """Adds what the C header `text` declares: consts[NAME] = int for `#define G2048_NAME value`,
    structs[c name] = a ctypes.Structure for `typedef struct g2048_x {...} g2048_x;`, protos[name] =
    (restype, argtypes) for `ret g2048_name(params);`.  Raises G2048Error on anything else."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+G2048_(\w+)[ \t]*(.*)$", text, flags=re.M):
        if value.strip():  # an include guard has none
            try:
                consts[name] = int(value.strip().strip("()").rstrip("uU"), 0)
            except ValueError:
                raise G2048Error(f"include/*.h: #define G2048_{name} {value.strip()}: not an integer") from None

    bodies = _STRUCT.findall(text)
    if len(bodies) != len(re.findall(r"typedef\s+struct\s+\w+\s*\{", text)):
        raise G2048Error("include/*.h: a `typedef struct ... {` that is not `typedef struct x {...} x;`")
    for tag, body, cname in bodies:
        if tag != cname or cname not in _STRUCT_NAMES:
            raise G2048Error(f"include/*.h: struct {tag} / {cname} has no Python name in _STRUCT_NAMES")
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            m = re.fullmatch(_TYPE + r"\b\s*(.+)", decl)
            if not m:
                raise G2048Error(f"include/*.h: {cname}: field `{decl}` not understood")
            for declarator in m.group(2).split(","):
                d = re.fullmatch(_STARS + r"(\w+)\s*(?:\[\s*(\w+)\s*\])?", declarator.strip())
                if not d:
                    raise G2048Error(f"include/*.h: {cname}: field `{decl}` not understood")
                stars, fname, dim = d.groups()
                ct = _ctype(m.group(1), stars, structs, f"{cname}: {decl}")
                if dim is not None:
                    size = int(dim) if dim.isdigit() else consts.get(dim.removeprefix("G2048_"))
                    if size is None:
                        raise G2048Error(f"include/*.h: {cname}: array size of `{decl}` is not known")
                    ct = ct * size
                fields.append((fname + "_" if keyword.iskeyword(fname) else fname, ct))
        structs[cname] = type(_STRUCT_NAMES[cname], (ctypes.Structure,),
                              {"_fields_": fields, "__doc__": f"struct {cname}", "__module__": __name__})

    # what is left are `;`-terminated statements: every one with a parenthesis must be a prototype
    rest = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{', "", _STRUCT.sub("", text), flags=re.M)
    found = set()
    for stmt in (" ".join(s.split()) for s in rest.split(";")):
        if "(" not in stmt:
            continue
        m = re.fullmatch(_TYPE + r"\b\s*" + _STARS + r"\b(g2048_[a-z0-9_]+) ?\(([^()]*)\)", stmt)
        if not m:
            raise G2048Error(f"include/*.h: `{stmt}` is not a prototype this binding understands")
        ret, stars, name, params = m.groups()
        argtypes = []
        for param in ([] if params.strip() == "void" else [p.strip() for p in params.split(",")]):
            a = re.fullmatch(_TYPE + r"\b\s*" + _STARS + r"\b(\w+)", param)
            if not a:
                raise G2048Error(f"include/*.h: {name}: parameter `{param}` not understood")
            argtypes.append(_ctype(a.group(1), a.group(2), structs, f"{name}: {param}"))
        protos[name] = (_ctype(ret, stars, structs, f"{name}: return type"), argtypes)
        found.add(name)
    declared = set(re.findall(r"\b(g2048_[a-z0-9_]+)\s*\(", text))
    if declared != found:
        raise G2048Error(f"include/*.h: prototypes not understood: {sorted(declared ^ found)}")


_CONSTS, _STRUCTS, _PROTOS = {}, {}, {}
for _h in HEADERS:
    _parse_header((INCLUDE_DIR / _h).read_text(), _CONSTS, _STRUCTS, _PROTOS)
if set(_STRUCTS) != set(_STRUCT_NAMES):
    raise G2048Error(f"include/*.h declares no struct {sorted(set(_STRUCT_NAMES) - set(_STRUCTS))}")
globals().update(_CONSTS)  # UP .. RIGHT, RNG_*, OPT_*, FLAG_*, DTYPE_*, RTG_STATE_DOUBLES, DY_MAX_P, COLSUM_*
globals().update({c.__name__: c for c in _STRUCTS.values()})  # Rng, RewardCfg, ... (_STRUCT_NAMES)
FLAG_LEGAL = _CONSTS["FLAG_LEGAL_MASK"]

_lib = None


def load(path: str | os.PathLike | None = None) -> ctypes.CDLL:
    """Load libg2048.so (no GPU needed to load; every compute call needs one) and bind every prototype
    of the headers."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path else LIB_PATH
    if not p.exists():
        raise G2048Error(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                         f"or `make -C 2048-ppo_amd/csrc`")
    L = ctypes.CDLL(str(p))
    for name, (res, args) in _PROTOS.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            if path is None:
                raise
            continue  # an older build loaded for an A/B timing: entry points it lacks stay unbound
        fn.restype, fn.argtypes = res, args
    if path is None:
        _lib = L
    return L


def _call(name: str, *args):
    """Calls the status-returning entry point `name`; a non-zero status raises."""
    status = getattr(load(), name)(*args)
    if status != 0:
        raise G2048Error(f"{name} failed with status {status}")


def _stream(t: torch.Tensor):
    if not t.is_cuda:
        raise G2048Error(f"tensor on {t.device}: libg2048 kernels need a ROCm device tensor (no CPU path)")
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _dev(t: torch.Tensor | None, dtype=None, name="tensor"):
    if t is None:
        return None
    if not t.is_cuda:
        raise G2048Error(f"{name} must be a ROCm device tensor (got {t.device}); there is no CPU path")
    if dtype is not None and t.dtype != dtype:
        raise G2048Error(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise G2048Error(f"{name} must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


def make_rng(mode=RNG_PHILOX, seed=0, counter=0, env_base=0, counter_dev=None, mt_state=None, inject=None) -> Rng:
    return Rng(mode, env_base, seed & (2**64 - 1), counter, _dev(counter_dev, torch.int64, "counter_dev"),
               _dev(mt_state, torch.int32, "mt_state"), _dev(inject, torch.int32, "inject"))


# ------------------------------------------------------------------------------- wrappers ------
def mt_seed(mt_state: torch.Tensor, seeds: torch.Tensor):
    n = seeds.numel()
    _call("g2048_mt_seed", _stream(seeds), _dev(mt_state, torch.int32, "mt_state"), _dev(seeds, torch.int64, "seeds"),
          n)


def env_reset(boards: torch.Tensor, flags: torch.Tensor | None, rng: Rng, where: torch.Tensor | None = None):
    _call("g2048_env_reset", _stream(boards), _dev(boards, torch.int8, "boards"), _dev(flags, torch.uint8, "flags"),
          _dev(where, torch.uint8, "where"), boards.shape[0], ctypes.byref(rng))


def env_step(boards_in, boards_out, actions_in, actions_out, points, max_tile, pot, flags, rng: Rng, options=0):
    n = boards_in.shape[0]
    _call("g2048_env_step", _stream(boards_in), _dev(boards_in, torch.int8, "boards_in"),
          _dev(boards_out, torch.int8, "boards_out"), _dev(actions_in, torch.uint8, "actions_in"),
          _dev(actions_out, torch.uint8, "actions_out"), _dev(points, torch.int32, "points"),
          _dev(max_tile, torch.int8, "max_tile"), _dev(pot, torch.int8, "pot"), _dev(flags, torch.uint8, "flags"), n,
          ctypes.byref(rng), options)


def env_rollout_random(boards, steps, traj_boards, traj_actions, traj_points, traj_pot, traj_flags, rng: Rng,
                       ticket=None):
    """ticket (a zero-filled int32 device word): the launch also advances rng's device counter by `steps`
    (g2048_env_rollout_random_adv: no counter-bump kernel between consecutive launches)."""
    args = (_stream(boards), _dev(boards, torch.int8, "boards"), boards.shape[0], steps,
            _dev(traj_boards, torch.int8, "traj_boards"), _dev(traj_actions, torch.uint8, "traj_actions"),
            _dev(traj_points, torch.int32, "traj_points"), _dev(traj_pot, torch.int8, "traj_pot"),
            _dev(traj_flags, torch.uint8, "traj_flags"), ctypes.byref(rng))
    if ticket is None:
        _call("g2048_env_rollout_random", *args)
    else:
        _call("g2048_env_rollout_random_adv", *args, _dev(ticket, torch.int32, "ticket"))


def env_rollout_form(n: int, steps: int) -> int:
    """The kernel env_rollout_random launches for n boards x steps: ROLLOUT_FORM_MFMA | ROLLOUT_FORM_WIDE
    bits, or EINVAL for a shape it refuses (g2048_env_rollout_form: host only, no device)."""
    return int(load().g2048_env_rollout_form(int(n), int(steps)))


def env_rollout_force_wide(on: bool) -> bool:
    """Test only: every later env_rollout_random launch takes the wide record addressing (True) or the
    form of its shape again (False).  Returns the previous setting."""
    return bool(load().g2048_env_rollout_force_wide(int(bool(on))))


def mc_search_workspace_bytes(n: int, playouts: int) -> int:
    return int(load().g2048_mc_search_workspace_bytes(int(n), int(playouts)))


def mc_search(boards, playouts: int, depth: int, rng: Rng, score_sum, move_sum=None, legal=None, best=None,
              workspace=None):
    """Monte-Carlo playout search (g2048_mc_search): boards int8 [n, 16] -> score_sum int64 [n, 4],
    move_sum int64 [n, 4], legal / best uint8 [n] (the last three optional).  workspace: a uint8 device
    tensor of mc_search_workspace_bytes(n, playouts) bytes (zero-filled by the call)."""
    n = boards.shape[0]
    for t, nm, k in ((score_sum, "score_sum", 4 * n), (move_sum, "move_sum", 4 * n), (legal, "legal", n),
                     (best, "best", n)):
        if t is not None and t.numel() < k:
            raise G2048Error(f"mc_search: {nm} holds {t.numel()} elements, needs {k}")
    if workspace is None:
        raise G2048Error("mc_search: a workspace of mc_search_workspace_bytes(n, playouts) bytes is required")
    _call("g2048_mc_search", _stream(boards), _dev(boards, torch.int8, "boards"), n, int(playouts), int(depth),
          ctypes.byref(rng), _dev(score_sum, torch.int64, "score_sum"), _dev(move_sum, torch.int64, "move_sum"),
          _dev(legal, torch.uint8, "legal"), _dev(best, torch.uint8, "best"), _dev(workspace, torch.uint8, "workspace"),
          workspace.numel())


def expectimax_workspace_bytes(n: int, depth: int, form: int = EMAX_AUTO) -> int:
    """0 for arguments g2048_expectimax would refuse."""
    return int(load().g2048_expectimax_workspace_bytes(int(n), int(depth), int(form)))


def expectimax(boards, depth: int, weights, value, leaves=None, legal=None, best=None, workspace=None,
               form: int = EMAX_AUTO):
    """Exact expectimax search (g2048_expectimax): boards int8 [n, 16], weights = (w_points, w_mono,
    w_empt) -> value int64 [n, 4] (-1: illegal), leaves int64 [n, 4], legal / best uint8 [n] (the last
    three optional).  workspace: a uint8 device tensor of expectimax_workspace_bytes(n, depth, form)
    bytes (zero-filled by the call)."""
    n = boards.shape[0]
    for t, nm, k in ((value, "value", 4 * n), (leaves, "leaves", 4 * n), (legal, "legal", n), (best, "best", n)):
        if t is not None and t.numel() < k:
            raise G2048Error(f"expectimax: {nm} holds {t.numel()} elements, needs {k}")
    if workspace is None:
        raise G2048Error("expectimax: a workspace of expectimax_workspace_bytes(n, depth, form) bytes is required")
    w_points, w_mono, w_empt = (int(x) for x in weights)
    _call("g2048_expectimax", _stream(boards), _dev(boards, torch.int8, "boards"), n, int(depth), w_points, w_mono,
          w_empt, int(form), _dev(value, torch.int64, "value"), _dev(leaves, torch.int64, "leaves"),
          _dev(legal, torch.uint8, "legal"), _dev(best, torch.uint8, "best"), _dev(workspace, torch.uint8, "workspace"),
          workspace.numel())


def make_ntuple_net(cells, weights: torch.Tensor, stage_map: int = 0):
    """The host struct of an n-tuple network: cells = T tuples of K cell indices (4 row + col), weights the
    device int32 tensor of its table entries.  stage_map 0: an NtNet, the one-stage net of T x 16^K weights.
    Otherwise an NtStagedNet of G x T x 16^K weights, stage_map the stage of every largest exponent: every
    ntuple_* wrapper below takes either and calls the entry point of its kind.  Raises for a net the library
    would refuse."""
    cells = [[int(c) for c in tup] for tup in cells]
    T, K = len(cells), len(cells[0]) if cells else 0
    if not 1 <= T <= NT_MAX_TUPLES or not 1 <= K <= NT_MAX_LEN or any(len(tup) != K for tup in cells):
        raise G2048Error(f"ntuple: 1..{NT_MAX_TUPLES} tuples of one length in 1..{NT_MAX_LEN}, got {cells}")
    flat = [c for tup in cells for c in tup]
    stage_map = int(stage_map)
    if not 0 <= stage_map < 1 << 64:
        raise G2048Error(f"ntuple: stage_map must fit 64 bits, got {stage_map}")
    net = NtNet(T, K, (ctypes.c_int32 * (NT_MAX_TUPLES * NT_MAX_LEN))(*flat), _dev(weights, torch.int32, "weights"))
    if stage_map == 0:
        count = int(load().g2048_ntuple_weight_count(ctypes.byref(net)))
    else:
        net = NtStagedNet(net, stage_map)
        count = int(load().g2048_ntuple_staged_weight_count(ctypes.byref(net)))
    if count == 0:
        raise G2048Error(f"ntuple: cells {cells} or stage_map {stage_map:#x} are refused (cells 0..15, distinct "
                         f"within a tuple; weights 16-B aligned; stages from 0, each the one before or one more)")
    if weights.numel() != count:
        raise G2048Error(f"ntuple: weights hold {weights.numel()} elements, the net needs {count}")
    return net


def _nt_entry(net, call: str) -> str:
    """The entry point `call` for the kind of net: g2048_ntuple_<call> or its twin on a staged net."""
    return f"g2048_ntuple_staged_{call}" if isinstance(net, NtStagedNet) else f"g2048_ntuple_{call}"


def _ntuple_weight_count(net) -> int:
    """G x T x 16^K of a net make_ntuple_net accepted."""
    if isinstance(net, NtStagedNet):
        return (1 + (net.stage_map >> 60)) * (net.net.num_tuples << (4 * net.net.tuple_len))
    return net.num_tuples << (4 * net.tuple_len)


def _staged(net) -> NtStagedNet:
    """The net as the staged entry points take it: a one-stage NtNet is the staged net with the map 0."""
    return net if isinstance(net, NtStagedNet) else NtStagedNet(net, 0)


def ntuple_stage(net, boards, out):
    """out uint8 [n] = stage(boards[i]) (g2048_ntuple_stage)."""
    n = boards.shape[0]
    if out is None or out.numel() < n:
        raise G2048Error(f"ntuple_stage: out holds {None if out is None else out.numel()} elements, needs {n}")
    _call("g2048_ntuple_stage", _stream(boards), ctypes.byref(_staged(net)), _dev(boards, torch.int8, "boards"),
          _dev(out, torch.uint8, "out"), n)


def ntuple_downgrade(boards, out, shift, from_exp: int, lo_exp: int, rounds: int):
    """out int8 [n, 16] = boards after at most `rounds` rounds of tile-downgrading, shift uint8 [n] (or None) the
    rounds applied (g2048_ntuple_downgrade).  out may be boards itself."""
    n = boards.shape[0]
    if out is None or out.numel() < 16 * n:
        raise G2048Error(f"ntuple_downgrade: out holds {None if out is None else out.numel()} elements, needs {16 * n}")
    if shift is not None and shift.numel() < n:
        raise G2048Error(f"ntuple_downgrade: shift holds {shift.numel()} elements, needs {n}")
    _call("g2048_ntuple_downgrade", _stream(boards), _dev(boards, torch.int8, "boards"), _dev(out, torch.int8, "out"),
          _dev(shift, torch.uint8, "shift"), n, int(from_exp), int(lo_exp), int(rounds))


def ntuple_promote(net, src: int, dst: int, device=None):
    """W[dst] += W[src], the tables of two stages of the net (g2048_ntuple_promote), on torch's current stream
    of `device` (the device of the net's weights; None: the current device)."""
    _call("g2048_ntuple_promote", ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream),
          ctypes.byref(_staged(net)),
          int(src), int(dst))


def ntuple_promote_from(net, src: int, dst: int, base: int, device=None):
    """W[dst] += W[src] - base, the promotion over the start `base` of the tables (g2048_ntuple_promote_from), on
    torch's current stream of `device` as ntuple_promote."""
    if not -(1 << 31) <= int(base) < 1 << 31:
        raise G2048Error(f"ntuple_promote_from: base must be an int32, got {base}")
    _call("g2048_ntuple_promote_from", ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream),
          ctypes.byref(_staged(net)), int(src), int(dst), int(base))


def ntuple_fill(net, w0: int, device=None):
    """Every weight of the net = w0, any int32 (g2048_ntuple_fill, or its twin on a staged net), on torch's current
    stream of `device` (the device of the net's weights; None: the current device)."""
    w0 = int(w0)
    if not -(1 << 31) <= w0 < 1 << 31:
        raise G2048Error(f"ntuple_fill: w0 must be an int32, got {w0}")
    _call(_nt_entry(net, "fill"), ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream), ctypes.byref(net), w0)


def ntuple_value(net, boards, value):
    """value int64 [n] = V(boards[i]) (g2048_ntuple_value)."""
    n = boards.shape[0]
    if value.numel() < n:
        raise G2048Error(f"ntuple_value: value holds {value.numel()} elements, needs {n}")
    _call(_nt_entry(net, "value"), _stream(boards), ctypes.byref(net), _dev(boards, torch.int8, "boards"),
          _dev(value, torch.int64, "value"), n)


def ntuple_choose(net, boards, q=None, legal=None, best=None):
    """The greedy choice (g2048_ntuple_choose): q int64 [n, 4] (INT64_MIN: illegal), legal / best uint8 [n];
    each optional, not all three."""
    n = boards.shape[0]
    for t, nm, k in ((q, "q", 4 * n), (legal, "legal", n), (best, "best", n)):
        if t is not None and t.numel() < k:
            raise G2048Error(f"ntuple_choose: {nm} holds {t.numel()} elements, needs {k}")
    _call(_nt_entry(net, "choose"), _stream(boards), ctypes.byref(net), _dev(boards, torch.int8, "boards"),
          _dev(q, torch.int64, "q"), _dev(legal, torch.uint8, "legal"), _dev(best, torch.uint8, "best"), n)


def ntuple_search_workspace_bytes(n: int, depth: int, form: int = EMAX_AUTO) -> int:
    """0 for arguments g2048_ntuple_search would refuse."""
    return int(load().g2048_ntuple_search_workspace_bytes(int(n), int(depth), int(form)))


def ntuple_search(net, boards, depth: int, q, leaves=None, legal=None, best=None, workspace=None,
                  form: int = EMAX_AUTO):
    """Expectimax search with the net at the leaves (g2048_ntuple_search): boards int8 [n, 16] -> q int64
    [n, 4] (INT64_MIN: illegal), leaves int64 [n, 4], legal / best uint8 [n] (the last three optional).
    workspace: a uint8 device tensor of ntuple_search_workspace_bytes(n, depth, form) bytes (zero-filled
    by the call)."""
    n = boards.shape[0]
    if q is None:
        raise G2048Error("ntuple_search: q is required")
    for t, nm, k in ((q, "q", 4 * n), (leaves, "leaves", 4 * n), (legal, "legal", n), (best, "best", n)):
        if t is not None and t.numel() < k:
            raise G2048Error(f"ntuple_search: {nm} holds {t.numel()} elements, needs {k}")
    if workspace is None:
        raise G2048Error("ntuple_search: a workspace of ntuple_search_workspace_bytes(n, depth, form) bytes "
                         "is required")
    _call(_nt_entry(net, "search"), _stream(boards), ctypes.byref(net), _dev(boards, torch.int8, "boards"), n, int(depth),
          int(form), _dev(q, torch.int64, "q"), _dev(leaves, torch.int64, "leaves"), _dev(legal, torch.uint8, "legal"),
          _dev(best, torch.uint8, "best"), _dev(workspace, torch.uint8, "workspace"), workspace.numel())


def ntuple_td_workspace_bytes(n: int) -> int:
    """0 for an n g2048_ntuple_td would refuse."""
    return int(load().g2048_ntuple_td_workspace_bytes(int(n)))


def ntuple_td(net, boards, after, pending, run_score, steps: int, lr_shift: int, rng: Rng, stats=None,
              workspace=None):
    """`steps` afterstate TD(0) steps of the n envs on one net (g2048_ntuple_td): boards / after int8 [n, 16],
    pending uint8 [n], run_score int64 [n] carried; stats int64 [4] accumulated (optional); workspace: a
    uint8 device tensor of ntuple_td_workspace_bytes(n) bytes."""
    n = boards.shape[0]
    for t, nm, k in ((after, "after", 16 * n), (pending, "pending", n), (run_score, "run_score", n), (stats, "stats", 4)):
        if t is not None and t.numel() < k:
            raise G2048Error(f"ntuple_td: {nm} holds {t.numel()} elements, needs {k}")
    if workspace is None:
        raise G2048Error("ntuple_td: a workspace of ntuple_td_workspace_bytes(n) bytes is required")
    _call(_nt_entry(net, "td"), _stream(boards), ctypes.byref(net), _dev(boards, torch.int8, "boards"),
          _dev(after, torch.int8, "after"), _dev(pending, torch.uint8, "pending"),
          _dev(run_score, torch.int64, "run_score"), n, int(steps), int(lr_shift), ctypes.byref(rng),
          _dev(stats, torch.int64, "stats"), _dev(workspace, torch.uint8, "workspace"), workspace.numel())


def ntuple_tc_workspace_bytes(n: int) -> int:
    """0 for an n g2048_ntuple_tc would refuse."""
    return int(load().g2048_ntuple_tc_workspace_bytes(int(n)))


def ntuple_tc(net, tc, boards, after, pending, run_score, steps: int, lr_shift: int, rng: Rng, stats=None,
              workspace=None):
    """`steps` temporal-coherence steps of the n envs on one net (g2048_ntuple_tc): ntuple_td's arguments and
    tc, the int64 device tensor [G, T, 16^K, 2] of the accumulators (E, A) of the net's weights, on the
    device of boards; workspace: a uint8 device tensor of ntuple_tc_workspace_bytes(n) bytes."""
    n = boards.shape[0]
    count = 2 * _ntuple_weight_count(net)  # two int64 per weight
    if tc is None or tc.dtype != torch.int64 or tc.numel() != count or tc.device != boards.device:
        raise G2048Error(f"ntuple_tc: tc must be int64 with {count} elements on {boards.device}, got "
                         f"{None if tc is None else (tc.dtype, tc.numel(), tc.device)}")
    for t, nm, k in ((after, "after", 16 * n), (pending, "pending", n), (run_score, "run_score", n), (stats, "stats", 4)):
        if t is not None and t.numel() < k:
            raise G2048Error(f"ntuple_tc: {nm} holds {t.numel()} elements, needs {k}")
    if workspace is None:
        raise G2048Error("ntuple_tc: a workspace of ntuple_tc_workspace_bytes(n) bytes is required")
    _call(_nt_entry(net, "tc"), _stream(boards), ctypes.byref(net), _dev(tc, torch.int64, "tc"),
          _dev(boards, torch.int8, "boards"), _dev(after, torch.int8, "after"), _dev(pending, torch.uint8, "pending"),
          _dev(run_score, torch.int64, "run_score"), n, int(steps), int(lr_shift), ctypes.byref(rng),
          _dev(stats, torch.int64, "stats"), _dev(workspace, torch.uint8, "workspace"), workspace.numel())


def ntuple_lambda_workspace_bytes(n: int) -> int:
    """0 for an n g2048_ntuple_lambda would refuse."""
    return int(load().g2048_ntuple_lambda_workspace_bytes(int(n)))


def ntuple_lambda(net, tc, boards, after, hist, hist_len, pending, run_score, steps: int, lr_shift: int,
                  trace_len: int, lambda_shift: int, rng: Rng, stats=None, workspace=None):
    """`steps` TD(lambda) (tc None) or TC(lambda) steps of the n envs on one net (g2048_ntuple_lambda), lambda =
    2^-lambda_shift over a trace of trace_len after-states: ntuple_td's arguments, tc as ntuple_tc's or None,
    and the carried history hist int8 [trace_len, n, 16] / hist_len uint8 [n] (both may be None with
    trace_len 0); workspace: a uint8 device tensor of ntuple_lambda_workspace_bytes(n) bytes."""
    n, trace_len = boards.shape[0], int(trace_len)
    if tc is not None:
        count = 2 * _ntuple_weight_count(net)  # two int64 per weight
        if tc.dtype != torch.int64 or tc.numel() != count or tc.device != boards.device:
            raise G2048Error(f"ntuple_lambda: tc must be int64 with {count} elements on {boards.device}, got "
                             f"{(tc.dtype, tc.numel(), tc.device)}")
    if trace_len > 0 and (hist is None or hist_len is None):
        raise G2048Error(f"ntuple_lambda: trace_len {trace_len} needs hist and hist_len")
    for t, nm, k in ((after, "after", 16 * n), (hist, "hist", 16 * n * max(trace_len, 0)), (hist_len, "hist_len", n),
                     (pending, "pending", n), (run_score, "run_score", n), (stats, "stats", 4)):
        if t is not None and t.numel() < k:
            raise G2048Error(f"ntuple_lambda: {nm} holds {t.numel()} elements, needs {k}")
    if workspace is None:
        raise G2048Error("ntuple_lambda: a workspace of ntuple_lambda_workspace_bytes(n) bytes is required")
    _call(_nt_entry(net, "lambda"), _stream(boards), ctypes.byref(net), _dev(tc, torch.int64, "tc"),
          _dev(boards, torch.int8, "boards"), _dev(after, torch.int8, "after"), _dev(hist, torch.int8, "hist"),
          _dev(hist_len, torch.uint8, "hist_len"), _dev(pending, torch.uint8, "pending"),
          _dev(run_score, torch.int64, "run_score"), n, int(steps), int(lr_shift), trace_len, int(lambda_shift),
          ctypes.byref(rng), _dev(stats, torch.int64, "stats"), _dev(workspace, torch.uint8, "workspace"),
          workspace.numel())


def ntuple_carousel_workspace_bytes(n: int) -> int:
    """0 for an n g2048_ntuple_staged_carousel would refuse."""
    return int(load().g2048_ntuple_carousel_workspace_bytes(int(n)))


def ntuple_carousel(net, tc, boards, after, hist, hist_len, pending, run_score, steps: int, lr_shift: int,
                    trace_len: int, lambda_shift: int, rng: Rng, pool, valid, next_stage, origin, stats=None,
                    workspace=None):
    """`steps` carousel steps of the n envs on a net with stages (g2048_ntuple_staged_carousel): ntuple_lambda's
    arguments and the carried carousel state pool int8 [G, n, 16], valid uint8 [n, 16], next_stage / origin
    uint8 [n]; stats int64 [8] accumulated (optional); workspace: a uint8 device tensor of
    ntuple_carousel_workspace_bytes(n) bytes."""
    n, trace_len = boards.shape[0], int(trace_len)
    snet = _staged(net)
    count = _ntuple_weight_count(net)
    if tc is not None:
        if tc.dtype != torch.int64 or tc.numel() != 2 * count or tc.device != boards.device:  # two int64 per weight
            raise G2048Error(f"ntuple_carousel: tc must be int64 with {2 * count} elements on {boards.device}, got "
                             f"{(tc.dtype, tc.numel(), tc.device)}")
    if trace_len > 0 and (hist is None or hist_len is None):
        raise G2048Error(f"ntuple_carousel: trace_len {trace_len} needs hist and hist_len")
    if any(t is None for t in (pool, valid, next_stage, origin)):
        raise G2048Error("ntuple_carousel: pool, valid, next_stage and origin are required")
    G = 1 + ((int(snet.stage_map) >> 60) & 15)
    for t, nm, k in ((after, "after", 16 * n), (hist, "hist", 16 * n * max(trace_len, 0)), (hist_len, "hist_len", n),
                     (pending, "pending", n), (run_score, "run_score", n), (stats, "stats", 8),
                     (pool, "pool", 16 * n * G), (valid, "valid", 16 * n), (next_stage, "next_stage", n),
                     (origin, "origin", n)):
        if t is not None and t.numel() < k:
            raise G2048Error(f"ntuple_carousel: {nm} holds {t.numel()} elements, needs {k}")
    if workspace is None:
        raise G2048Error("ntuple_carousel: a workspace of ntuple_carousel_workspace_bytes(n) bytes is required")
    car = NtCarousel(_dev(pool, torch.int8, "pool"), _dev(valid, torch.uint8, "valid"),
                     _dev(next_stage, torch.uint8, "next_stage"), _dev(origin, torch.uint8, "origin"))
    _call("g2048_ntuple_staged_carousel", _stream(boards), ctypes.byref(snet), _dev(tc, torch.int64, "tc"),
          _dev(boards, torch.int8, "boards"), _dev(after, torch.int8, "after"), _dev(hist, torch.int8, "hist"),
          _dev(hist_len, torch.uint8, "hist_len"), _dev(pending, torch.uint8, "pending"),
          _dev(run_score, torch.int64, "run_score"), n, int(steps), int(lr_shift), trace_len, int(lambda_shift),
          ctypes.byref(rng), ctypes.byref(car), _dev(stats, torch.int64, "stats"),
          _dev(workspace, torch.uint8, "workspace"), workspace.numel())


def preview_points(boards, points4):
    _call("g2048_preview_points", _stream(boards), _dev(boards, torch.int8, "boards"),
          _dev(points4, torch.int32, "points4"), boards.shape[0])


def legal_mask(boards, flags):
    _call("g2048_legal_mask", _stream(boards), _dev(boards, torch.int8, "boards"), _dev(flags, torch.uint8, "flags"),
          boards.shape[0])


def obs_encode(boards, obs):
    dt = {torch.float32: DTYPE_F32, torch.bfloat16: DTYPE_BF16}.get(obs.dtype)
    if dt is None:
        raise G2048Error(f"obs dtype {obs.dtype} unsupported")
    _call("g2048_obs_encode", _stream(boards), _dev(boards, torch.int8, "boards"), _dev(obs, None, "obs"), dt,
          boards.shape[0])


def info_deltas(boards, actions, deltas, anchor=None):
    """boards int8 [n, 16], actions uint8 [n] -> deltas float64 [n, 5] (smoothness, corner, adjacency,
    chain, topological after - before the move), anchor int8 [n] (optional)."""
    n = boards.shape[0]
    _call("g2048_info_deltas", _stream(boards), _dev(boards, torch.int8, "boards"),
          _dev(actions, torch.uint8, "actions"), _dev(deltas, torch.float64, "deltas"),
          _dev(anchor, torch.int8, "anchor"), n)


def sample_actions(logits, flags, actions, logp, entropy, rng: Rng):
    n = flags.shape[0]
    stride = 0
    lp = None
    if logits is not None:
        if logits.dtype != torch.float32 or not logits.is_cuda or logits.stride(-1) != 1:
            raise G2048Error("logits must be float32 on device with unit inner stride")
        stride = logits.stride(0)
        lp = ctypes.c_void_p(logits.data_ptr())
    _call("g2048_sample_actions", _stream(flags), lp, stride, _dev(flags, torch.uint8, "flags"),
          _dev(actions, torch.uint8, "actions"), _dev(logp, torch.float32, "logp"),
          _dev(entropy, torch.float32, "entropy"), n, ctypes.byref(rng))


def rtg_workspace_bytes(n: int) -> int:
    return int(load().g2048_reward_rtg_workspace_bytes(n))


def rtg_prepare(state, cfg: RewardCfg):
    _call("g2048_rtg_prepare", _stream(state), _dev(state, torch.float64, "state"), ctypes.byref(cfg))


def reward_rtg(points, pot, flags, value, state, g_raw, g_norm, adv, partials, workspace, cfg: RewardCfg,
               reward=None):
    """reward (optional) float64 [T, n]: the per-step reward the scan used."""
    T, n = points.shape[0], points.shape[1]
    _call("g2048_reward_rtg_ex", _stream(points), _dev(points, torch.int32, "points"), _dev(pot, torch.int8, "pot"),
          _dev(flags, torch.uint8, "flags"), _dev(value, torch.float32, "value"), T, n, ctypes.byref(cfg),
          _dev(state, torch.float64, "state"), _dev(g_raw, torch.float32, "g_raw"),
          _dev(g_norm, torch.float32, "g_norm"), _dev(adv, torch.float32, "adv"),
          _dev(reward, torch.float64, "reward") if reward is not None else None,
          _dev(partials, torch.float64, "partials"), _dev(workspace, torch.uint8, "workspace"), workspace.numel())


def episode_scan(points, boards, max_tile, step_flags, run_score, run_max, scores, tiles):
    """points/max_tile/step_flags [T, n], boards [T, n, 16]; run_score int64 / run_max int32 [n] carried."""
    T, n = points.shape[0], points.shape[1]
    _call("g2048_episode_scan", _stream(points), _dev(points, torch.int32, "points"),
          _dev(boards, torch.int8, "boards"), _dev(max_tile, torch.int8, "max_tile"),
          _dev(step_flags, torch.uint8, "step_flags"), T, n, _dev(run_score, torch.int64, "run_score"),
          _dev(run_max, torch.int32, "run_max"), _dev(scores, torch.int64, "scores"), _dev(tiles, torch.int32, "tiles"))


def permutation(out, n: int, key=None, seed: int = 0, counter: int = 0):
    """out[:n] (int64, device) = a keyed random permutation of [0, n) (g2048_permutation); key: a
    device int64 [1] (e.g. drawn from the caller's generator: no host read) or None for (seed, counter)."""
    if out.numel() < n:
        raise G2048Error("permutation: out too small")
    _call("g2048_permutation", _stream(out), _dev(out, torch.int64, "out"), int(n), _dev(key, torch.int64, "key"),
          int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1))


ROLLOUT_STATS = 23  # g2048_rollout_stats' output vector


def rollout_stats_workspace_bytes(T: int, n: int) -> int:
    return int(load().g2048_rollout_stats_workspace_bytes(int(T), int(n)))


def rollout_stats(points, pot, step_flags, value, g_raw, g_norm, adv, boards, max_tile, episodic, cfg,
                  run_score, run_max, workspace, out):
    """The rollout metrics vector out [23] float32 (include/g2048.h g2048_rollout_stats).  points /
    step_flags / value / g_raw / g_norm / adv [T, n], pot [T, n, 4]; fixed horizon: boards [T, n, 16],
    max_tile [T, n], run_score / run_max [n] carried; episodic: boards [T + 1, n, 16] (the final board
    read), max_tile / run_* may be None.  cfg: RewardCfg.  workspace: a zero-filled uint8 tensor of
    rollout_stats_workspace_bytes(T, n) bytes, left zeroed."""
    T, n = points.shape[0], points.shape[1]
    _call("g2048_rollout_stats", _stream(points), _dev(points, torch.int32, "points"), _dev(pot, torch.int8, "pot"),
          _dev(step_flags, torch.uint8, "step_flags"), _dev(value, torch.float32, "value"),
          _dev(g_raw, torch.float32, "g_raw"), _dev(g_norm, torch.float32, "g_norm"), _dev(adv, torch.float32, "adv"),
          _dev(boards, torch.int8, "boards"), _dev(max_tile, torch.int8, "max_tile"), T, n, 1 if episodic else 0,
          ctypes.byref(cfg), _dev(run_score, torch.int64, "run_score"), _dev(run_max, torch.int32, "run_max"),
          _dev(workspace, torch.uint8, "workspace"), workspace.numel(), _dev(out, torch.float32, "out"))


def augment_workspace_bytes(k: int) -> int:
    return int(load().g2048_augment_workspace_bytes(int(k)))


def augment(boards, actions, legal, logp, adv, ret, n: int, k: int, seed: int, counter: int, workspace, count):
    """D4 up-sampling (train.py:774-881): appends the copies of k sampled rows of the pool after its
    n real rows; count (int64 [1], device) = n + copies.  Pool capacity >= n + 2k."""
    cap = boards.shape[0]
    for t, nm in ((actions, "actions"), (legal, "legal"), (logp, "logp"), (adv, "adv"), (ret, "ret")):
        if t.shape[0] != cap:
            raise G2048Error(f"augment: {nm} has {t.shape[0]} rows, boards {cap}")
    if k > 0 and cap < n + 2 * k:
        raise G2048Error(f"augment: pool capacity {cap} < n + 2k = {n + 2 * k}")
    _call("g2048_augment", _stream(boards), _dev(boards, torch.int8, "boards"), _dev(actions, torch.uint8, "actions"),
          _dev(legal, torch.uint8, "legal"), _dev(logp, torch.float32, "logp"), _dev(adv, torch.float32, "adv"),
          _dev(ret, torch.float32, "ret"), int(n), int(k), int(seed) & (2**64 - 1), int(counter) & (2**64 - 1),
          _dev(workspace, None, "workspace"), workspace.numel() * workspace.element_size(),
          _dev(count, torch.int64, "count"))


def rtg_finalize(state, partials, cfg: RewardCfg):
    _call("g2048_rtg_finalize", _stream(state), _dev(state, torch.float64, "state"),
          _dev(partials, torch.float64, "partials"), ctypes.byref(cfg))


# ------------------------------------------------------------- PPO update (g2048_ppo.h) -------
def make_dropout(p=0.0, layer=0, pass_=0, seed=0, counter=0, counter_dev=None) -> Dropout:
    return Dropout(float(p), layer, pass_, 0, seed & (2**64 - 1), counter,
                   _dev(counter_dev, torch.int64, "counter_dev"))


def obs_gather(boards, idx, obs):
    _call("g2048_obs_gather", _stream(idx), _dev(boards, torch.int8, "boards"), _dev(idx, torch.int64, "idx"),
          idx.shape[0], _dev(obs, torch.bfloat16, "obs"))


def ln_act_fwd(g, gamma, beta, res, y, mean, rstd, drop: Dropout | None = None):
    m, h = g.shape
    _call("g2048_ln_act_fwd", _stream(g), _dev(g, torch.bfloat16, "g"), _dev(gamma, torch.float32, "gamma"),
          _dev(beta, torch.float32, "beta"), _dev(res, torch.bfloat16, "res"), _dev(y, torch.bfloat16, "y"),
          _dev(mean, torch.float32, "mean"), _dev(rstd, torch.float32, "rstd"), m, h,
          ctypes.byref(drop) if drop is not None else None)


def ln_act_bwd_partials(m: int, h: int) -> int:
    return int(load().g2048_ln_act_bwd_partials(m, h))


def make_dy(dres=None, ps=(), head=None) -> Dy:
    """dy = dres + sum(ps) + heads; head = (dz, wa, wv) with wv None for a decoupled critic."""
    ps = [p for p in ps if p is not None]
    if len(ps) > DY_MAX_P:
        raise G2048Error(f"at most {DY_MAX_P} matmul gradients per LayerNorm backward")
    d = Dy()
    d.dres = _dev(dres, torch.float32, "dres")
    for i, p in enumerate(ps):
        d.p[i] = _dev(p, torch.bfloat16, f"p[{i}]")
    if head is not None:
        dz, wa, wv = head
        d.dz, d.wa, d.wv = _dev(dz, torch.float32, "dz"), _dev(wa, torch.float32, "wa"), _dev(wv, torch.float32, "wv")
    return d


def _defer(job):
    return ctypes.byref(job) if job is not None else None


def ln_act_bwd(dres_in, p_in, g, mean, rstd, gamma, beta, dg, dres_out, partials, dgamma, dbeta,
               drop: Dropout | None = None, head=None, dy: Dy | None = None, defer: ColsumJob | None = None):
    """LayerNorm/ReLU/dropout backward; the output gradient is `dy` (a Dy) or dres_in + p_in (+ head)."""
    m, h = g.shape
    if dy is None:
        dy = make_dy(dres_in, [p_in], head)
    _call("g2048_ln_act_bwd", _stream(g), ctypes.byref(dy), _dev(g, torch.bfloat16, "g"),
          _dev(mean, torch.float32, "mean"), _dev(rstd, torch.float32, "rstd"), _dev(gamma, torch.float32, "gamma"),
          _dev(beta, torch.float32, "beta"), _dev(dg, torch.bfloat16, "dg"), _dev(dres_out, torch.float32, "dres_out"),
          _dev(partials, torch.float32, "partials"), _dev(dgamma, torch.float32, "dgamma"),
          _dev(dbeta, torch.float32, "dbeta"), m, h, ctypes.byref(drop) if drop is not None else None, _defer(defer))


def ppo_head_partials(m: int, h: int) -> int:
    return int(load().g2048_ppo_head_partials(m, h))


def make_ppo_batch(idx, action, legal, old_logp, adv, ret, rows=None) -> PPOBatch:
    """rows (optional int64 device scalar): valid rows of a padded ragged minibatch."""
    return PPOBatch(_dev(idx, torch.int64, "idx"), _dev(action, torch.uint8, "action"),
                    _dev(legal, torch.uint8, "legal"), _dev(old_logp, torch.float32, "old_logp"),
                    _dev(adv, torch.float32, "adv"), _dev(ret, torch.float32, "ret"), _dev(rows, torch.int64, "rows"))


def ppo_head_loss(x, wa, ba, wv, bv, batch: PPOBatch, beta_dev, critic, clip_eps, decouple, masked, dx, partials,
                  dwa, dba, dwv, dbv, sums, dz=None, defer: ColsumJob | None = None):
    m, h = x.shape
    _call("g2048_ppo_head_loss", _stream(x), _dev(x, torch.bfloat16, "x"), _dev(wa, torch.float32, "wa"),
          _dev(ba, torch.float32, "ba"), _dev(wv, torch.float32, "wv"), _dev(bv, torch.float32, "bv"), m, h,
          ctypes.byref(batch), _dev(beta_dev, torch.float32, "beta"), float(critic), float(clip_eps),
          int(bool(decouple)), _dev(masked, torch.float32, "masked"), _dev(dx, torch.float32, "dx"),
          _dev(dz, torch.float32, "dz"), _dev(partials, torch.float32, "partials"), _dev(dwa, torch.float32, "dwa"),
          _dev(dba, torch.float32, "dba"), _dev(dwv, torch.float32, "dwv"), _dev(dbv, torch.float32, "dbv"),
          _dev(sums, torch.float32, "sums"), _defer(defer))


def mlp_fwd_kl_supported(n: int, k: int) -> bool:
    return n == 196 and k == 196


def mlp_fwd_kl(x, w, gamma, beta, drop, wa, ba, old_masked, partials, out, defer: ColsumJob | None = None, rows=None):
    """The KL re-forward's last ResidualBlock fused with the action head and the KL reduction."""
    m, k = x.shape
    _call("g2048_mlp_fwd_kl", _stream(x), _dev(x, torch.bfloat16, "x"), _dev(w, torch.bfloat16, "w"),
          _dev(gamma, torch.float32, "gamma"), _dev(beta, torch.float32, "beta"), m, w.shape[0], k,
          ctypes.byref(drop) if drop is not None else None, _dev(wa, torch.float32, "wa"),
          _dev(ba, torch.float32, "ba"), _dev(old_masked, torch.float32, "old_masked"), _dev(rows, torch.int64, "rows"),
          _dev(partials, torch.float32, "partials"), _dev(out, torch.float32, "out"), _defer(defer))


def ppo_head_kl(x, wa, ba, old_masked, partials, out, defer: ColsumJob | None = None, rows=None):
    m, h = x.shape
    _call("g2048_ppo_head_kl", _stream(x), _dev(x, torch.bfloat16, "x"), _dev(wa, torch.float32, "wa"),
          _dev(ba, torch.float32, "ba"), m, h, _dev(old_masked, torch.float32, "old_masked"),
          _dev(rows, torch.int64, "rows"), _dev(partials, torch.float32, "partials"), _dev(out, torch.float32, "out"),
          _defer(defer))


def mlp_pass_supported(hidden: int, num_layers: int) -> bool:
    """The fused train / KL passes (g2048_ppo_forward_loss / _kl) cover this GameMLP shape."""
    return bool(load().g2048_mlp_pass_supported(int(hidden), int(num_layers)))


def mlp_pass_partials(m: int, train: bool) -> int:
    return int(load().g2048_mlp_pass_partials(int(m), int(bool(train))))


def head_split_bytes(hidden: int) -> int:
    return int(load().g2048_head_split_bytes(int(hidden)))


def head_split(wa, wv, frag):
    """frag (uint8 device buffer of head_split_bytes(h)) <- the 3-term bf16 split of [wa; wv]."""
    h = wa.shape[1]
    _call("g2048_head_split", _stream(wa), _dev(wa, torch.float32, "wa"), _dev(wv, torch.float32, "wv"), h,
          _dev(frag, None, "frag"))


def make_mlp_pass(boards, batch: PPOBatch, m: int, w_stem, w_blocks, gammas, betas, head_frag, ba, bv=None,
                  drops=(None, None), beta_dev=None, critic=0.0, clip_eps=0.2, decouple=False, x0=None,
                  g=(None, None, None), h=(None, None, None), mean=(None, None, None), rstd=(None, None, None),
                  masked=None, dz=None, dz_bf16=None, partials=None, keep=None, idx_offset=None) -> MlpPassArgs:
    """struct g2048_mlp_pass_args for g2048_ppo_forward_loss / g2048_ppo_forward_kl (GameMLP, 2 blocks).
    keep (train pass, optional): int64 [2, m, 4] out, the blocks' dropout keep bits for the backward."""
    a = MlpPassArgs()
    a.boards = _dev(boards, torch.int8, "boards")
    a.batch = batch
    a.m = int(m)
    a.hidden = int(w_stem.shape[0])
    a.decouple_critic = int(bool(decouple))
    a.w_stem = _dev(w_stem, torch.bfloat16, "w_stem")
    for i, w in enumerate(w_blocks):
        a.w_block[i] = _dev(w, torch.bfloat16, f"w_block[{i}]")
    for i, (gm, bt) in enumerate(zip(gammas, betas)):
        a.ln_gamma[i], a.ln_beta[i] = _dev(gm, torch.float32, "gamma"), _dev(bt, torch.float32, "beta")
    a.head_frag = _dev(head_frag, None, "head_frag")
    a.ba, a.bv = _dev(ba, torch.float32, "ba"), _dev(bv, torch.float32, "bv")
    for i, d in enumerate(drops):
        if d is not None:
            a.drop[i] = d
    a.beta_dev = _dev(beta_dev, torch.float32, "beta_dev")
    a.critic, a.clip_eps = float(critic), float(clip_eps)
    a.x0 = _dev(x0, torch.bfloat16, "x0")
    for i in range(3):
        a.g[i] = _dev(g[i], torch.bfloat16, f"g[{i}]")
        a.h[i] = _dev(h[i], torch.bfloat16, f"h[{i}]")
        a.mean[i] = _dev(mean[i], torch.float32, f"mean[{i}]")
        a.rstd[i] = _dev(rstd[i], torch.float32, f"rstd[{i}]")
    a.masked = _dev(masked, torch.float32, "masked")
    a.dz = _dev(dz, torch.float32, "dz")
    a.dz_bf16 = _dev(dz_bf16, torch.bfloat16, "dz_bf16")
    a.partials = _dev(partials, torch.float32, "partials")
    a.keep = _dev(keep, torch.int64, "keep")
    a.idx_offset = _dev(idx_offset, torch.int64, "idx_offset")
    return a


def ppo_forward_loss(args: MlpPassArgs, dba, dbv, sums, defer: ColsumJob | None = None, like=None):
    """The fused train pass (obs -> GameMLP -> heads -> PPO loss / dz) of one minibatch."""
    _call("g2048_ppo_forward_loss", _stream(like if like is not None else dba), ctypes.byref(args),
          _dev(dba, torch.float32, "dba"), _dev(dbv, torch.float32, "dbv"), _dev(sums, torch.float32, "sums"),
          _defer(defer))


def ppo_forward_kl(args: MlpPassArgs, out, defer: ColsumJob | None = None):
    """The fused KL re-forward of one minibatch: out[2] = {sum KL, max KL}."""
    _call("g2048_ppo_forward_kl", _stream(out), ctypes.byref(args), _dev(out, torch.float32, "out"), _defer(defer))


def ppo_forward_kl_stats(args: MlpPassArgs, sums, grad_norm, beta_dev, critic: float, m: int, stats, sync,
                         counter=None, rows=None, idx_offset=None, idx_step: int = 0):
    """The fused KL re-forward whose last block also accumulates the minibatch statistics
    (g2048_ppo_stats folded in); sync: a zeroed int32 device word kept across calls."""
    st = PPOStatsArgs(_dev(sums, torch.float32, "sums"), _dev(grad_norm, torch.float32, "grad_norm"),
                      _dev(beta_dev, torch.float32, "beta_dev"), _dev(rows, torch.int64, "rows"),
                      _dev(stats, torch.float32, "stats"), _dev(counter, torch.int64, "counter"),
                      _dev(sync, torch.int32, "sync"), float(critic), 0, int(m),
                      _dev(idx_offset, torch.int64, "idx_offset"), int(idx_step))
    _call("g2048_ppo_forward_kl_stats", _stream(stats), ctypes.byref(args), ctypes.byref(st))


def mlp_back_partials(m: int, h: int) -> int:
    return int(load().g2048_mlp_back_partials(int(m), int(h)))


def make_mlp_back(m: int, w_blocks, gammas, betas, wa, wv, dz, g, mean, rstd, drops=(None, None), dg=(None,) * 3,
                  partials=None, p_out=(None, None), keep=None) -> MlpBackArgs:
    """struct g2048_mlp_back_args for g2048_ppo_backward (GameMLP, 2 blocks).  keep: the train pass's
    keep bits (make_mlp_pass(keep=...)) for the same drops, read instead of re-drawing the masks."""
    a = MlpBackArgs()
    a.m = int(m)
    a.hidden = int(w_blocks[0].shape[0])
    for i, w in enumerate(w_blocks):
        a.w_block[i] = _dev(w, torch.bfloat16, f"w_block[{i}]")
    for i, (gm, bt) in enumerate(zip(gammas, betas)):
        a.ln_gamma[i], a.ln_beta[i] = _dev(gm, torch.float32, "gamma"), _dev(bt, torch.float32, "beta")
    a.wa, a.wv = _dev(wa, torch.float32, "wa"), _dev(wv, torch.float32, "wv")
    a.dz = _dev(dz, torch.float32, "dz")
    for i in range(3):
        a.g[i] = _dev(g[i], torch.bfloat16, f"g[{i}]")
        a.mean[i] = _dev(mean[i], torch.float32, f"mean[{i}]")
        a.rstd[i] = _dev(rstd[i], torch.float32, f"rstd[{i}]")
        a.dg[i] = _dev(dg[i], torch.bfloat16, f"dg[{i}]")
    for i in range(2):
        a.p_out[i] = _dev(p_out[i], torch.bfloat16, f"p_out[{i}]")
    for i, d in enumerate(drops):
        if d is not None:
            a.drop[i] = d
    a.partials = _dev(partials, torch.float32, "partials")
    a.keep = _dev(keep, torch.int64, "keep")
    return a


def mlp_wgrad_partials(m: int, h: int) -> int:
    return int(load().g2048_mlp_wgrad_partials(int(m), int(h)))


def mlp_wgrad(m: int, dz_bf16, h2, dg, x, partials, out_head, out_w, defer=None):
    """The four weight gradients of the GameMLP minibatch in one launch (g2048_mlp_wgrad):
    out_head [16, h] = dz_bf16^T h2, out_w[0] [h, 48] = dg[0]^T x[0], out_w[l] [h, h] = dg[l]^T x[l];
    defer: a list of four ColsumJob (head, stem, block 1, block 2) filled instead of summing."""
    a = MlpWgradArgs()
    a.m = int(m)
    a.hidden = int(h2.shape[1])
    a.dz_bf16 = _dev(dz_bf16, torch.bfloat16, "dz_bf16")
    a.h2 = _dev(h2, torch.bfloat16, "h2")
    for i in range(3):
        a.dg[i] = _dev(dg[i], torch.bfloat16, f"dg[{i}]")
        a.x[i] = _dev(x[i], torch.bfloat16, f"x[{i}]")
    a.partials = _dev(partials, torch.float32, "partials")
    vp = ctypes.c_void_p
    outs = (vp * 3)(*[_dev(t, torch.float32, "out_w") for t in out_w])
    jobs = (ColsumJob * 4)() if defer is not None else None
    _call("g2048_mlp_wgrad", _stream(out_head), ctypes.byref(a), _dev(out_head, torch.float32, "out_head"), outs, jobs)
    if defer is not None:
        for i in range(4):
            defer[i] = jobs[i]


def ppo_backward(args: MlpBackArgs, dgamma, dbeta, defer=None, like=None):
    """The fused MLP backward of one minibatch (three dG, the LayerNorm affine gradients); defer: a
    list of three ColsumJob filled instead of summing at once."""
    vp = ctypes.c_void_p
    dgp = (vp * 3)(*[_dev(t, torch.float32, "dgamma") for t in dgamma])
    dbp = (vp * 3)(*[_dev(t, torch.float32, "dbeta") for t in dbeta])
    jobs = None
    if defer is not None:
        jobs = (ColsumJob * 3)()
    _call("g2048_ppo_backward", _stream(like if like is not None else dgamma[0]), ctypes.byref(args), dgp, dbp, jobs)
    if defer is not None:
        for i in range(3):
            defer[i] = jobs[i]


def dropout_mask(m: int, h: int, drop: Dropout, mask):
    _call("g2048_dropout_mask", _stream(mask), m, h, ctypes.byref(drop), _dev(mask, torch.uint8, "mask"))


def wgrad_partials(m: int, n1: int, n2: int) -> int:
    """Scratch floats of wgrad (0 = shape not supported by the MFMA kernel)."""
    return int(load().g2048_wgrad_partials(m, n1, n2))


def wgrad(a, b, partials, out, defer: ColsumJob | None = None):
    """out[n1, n2] = a^T b for bf16 a [m, n1], b [m, n2]; fp32 out."""
    m, n1 = a.shape
    n2 = b.shape[1]
    if b.shape[0] != m or tuple(out.shape) != (n1, n2):
        raise G2048Error(f"wgrad shapes: a {tuple(a.shape)} b {tuple(b.shape)} out {tuple(out.shape)}")
    _call("g2048_wgrad", _stream(a), _dev(a, torch.bfloat16, "a"), _dev(b, torch.bfloat16, "b"), m, n1, n2,
          _dev(partials, torch.float32, "partials"), _dev(out, torch.float32, "out"), _defer(defer))


def wgrad_pair_partials(m: int, n1: int, n2: int) -> int:
    return int(load().g2048_wgrad_pair_partials(m, n1, n2))


def wgrad_pair(a0, b0, a1, b1, partials0, partials1, out0, out1, defer=None):
    """out0 = a0^T b0 and out1 = a1^T b1 (same shapes) in one launch; defer: a list of two ColsumJob."""
    m, n1 = a0.shape
    n2 = b0.shape[1]
    for a, b, o in ((a0, b0, out0), (a1, b1, out1)):
        if a.shape != (m, n1) or b.shape != (m, n2) or tuple(o.shape) != (n1, n2):
            raise G2048Error("wgrad_pair shapes")
    jobs = (ColsumJob * 2)() if defer is not None else None
    _call("g2048_wgrad_pair", _stream(a0), *[_dev(t, torch.bfloat16, "a/b") for t in (a0, b0, a1, b1)], m, n1, n2,
          _dev(partials0, torch.float32, "partials0"), _dev(partials1, torch.float32, "partials1"),
          _dev(out0, torch.float32, "out0"), _dev(out1, torch.float32, "out1"), jobs)
    if defer is not None:
        defer[0], defer[1] = jobs[0], jobs[1]


def colsum_batch(jobs):
    """Performs deferred column sums (ColsumJob list, at most COLSUM_MAX_JOBS) in one launch; `jobs`
    may also be a ctypes array built once (graph-captured callers)."""
    n = len(jobs)
    if n > COLSUM_MAX_JOBS:
        raise G2048Error(f"at most {COLSUM_MAX_JOBS} column-sum jobs per launch")
    if not isinstance(jobs, ctypes.Array):
        jobs = (ColsumJob * max(1, n))(*jobs)
    stream = torch.cuda.current_stream().cuda_stream
    _call("g2048_colsum_batch", ctypes.c_void_p(stream), jobs, n)


def colsum_batch_sq(jobs, sq, tick=None):
    """colsum_batch + the gradient norm's partials: sq (fp32, COLSUM_SQ_MAX) <- per-block sums of
    squares of the segments marked in each job's pad_ (bit k = segment k is gradient), *tick += 1."""
    n = len(jobs)
    if n > COLSUM_MAX_JOBS:
        raise G2048Error(f"at most {COLSUM_MAX_JOBS} column-sum jobs per launch")
    if not isinstance(jobs, ctypes.Array):
        jobs = (ColsumJob * max(1, n))(*jobs)
    stream = torch.cuda.current_stream().cuda_stream
    _call("g2048_colsum_batch_sq", ctypes.c_void_p(stream), jobs, n, _dev(sq, torch.float32, "sq"), sq.numel(),
          _dev(tick, torch.float32, "tick"))


def colsum_batch_blocks(jobs) -> int:
    if not isinstance(jobs, ctypes.Array):
        jobs = (ColsumJob * max(1, len(jobs)))(*jobs)
    return int(load().g2048_colsum_batch_blocks(jobs, len(jobs)))


# ------------------------------------------------------------- optimizer step -------------------
def grad_clip(grad, max_norm: float, norm_out, coef_out, partials):
    """partials: >= 64 float32 of scratch."""
    _call("g2048_grad_clip", _stream(grad), _dev(grad, torch.float32, "grad"), grad.numel(), float(max_norm),
          _dev(norm_out, torch.float32, "norm_out"), _dev(coef_out, torch.float32, "coef_out"),
          _dev(partials, torch.float32, "partials"))


def muon_supported(rows: int, cols: int) -> bool:
    return bool(load().g2048_muon_supported(rows, cols))


def muon_step(mats, lr_dev, clip_coef_dev, cfg: MuonCfg, stream_tensor):
    """mats: a ctypes array of MuonMatrix (built once; device pointers stay valid)."""
    _call("g2048_muon_step", _stream(stream_tensor), mats, len(mats), _dev(lr_dev, torch.float32, "lr"),
          _dev(clip_coef_dev, torch.float32, "clip"), ctypes.byref(cfg))


def grad_sumsq(grad, partials):
    _call("g2048_grad_sumsq", _stream(grad), _dev(grad, torch.float32, "grad"), grad.numel(),
          _dev(partials, torch.float32, "partials"))


def muon_step_clip(mats, lr_dev, partials, max_norm: float, norm_out, coef_out, cfg: MuonCfg):
    """Muon with the gradient clip folded in (partials from grad_sumsq; norm / coef published)."""
    _call("g2048_muon_step_clip", _stream(lr_dev), mats, len(mats), _dev(lr_dev, torch.float32, "lr"),
          _dev(partials, torch.float32, "partials"), float(max_norm), _dev(norm_out, torch.float32, "norm_out"),
          _dev(coef_out, torch.float32, "coef_out"), ctypes.byref(cfg))


def grad_sumsq_tick(grad, partials, step_dev):
    """grad_sumsq + the optimizer's device step count += 1 (one launch)."""
    _call("g2048_grad_sumsq_tick", _stream(grad), _dev(grad, torch.float32, "grad"), grad.numel(),
          _dev(partials, torch.float32, "partials"), _dev(step_dev, torch.float32, "step"))


def muon_adamw_step_clip(mats, groups, lr_dev, step_dev, partials, max_norm: float, norm_out, coef_out, cfg: MuonCfg,
                         beta1, beta2, eps, adam_weight_decay):
    """muon_step_clip with the AdamW update of the 1-D groups in the same launch."""
    _call("g2048_muon_adamw_step_clip", _stream(lr_dev), mats, len(mats), groups,
          len(groups) if groups is not None else 0, _dev(lr_dev, torch.float32, "lr"),
          _dev(step_dev, torch.float32, "step"), _dev(partials, torch.float32, "partials"), float(max_norm),
          _dev(norm_out, torch.float32, "norm_out"), _dev(coef_out, torch.float32, "coef_out"), ctypes.byref(cfg),
          float(beta1), float(beta2), float(eps), float(adam_weight_decay))


def adamw_step(groups, lr_dev, step_dev, clip_coef_dev, beta1, beta2, eps, weight_decay):
    _call("g2048_adamw_step", _stream(lr_dev), groups, len(groups), _dev(lr_dev, torch.float32, "lr"),
          _dev(step_dev, torch.float32, "step"), _dev(clip_coef_dev, torch.float32, "clip"), float(beta1), float(beta2),
          float(eps), float(weight_decay))


def mlp_fwd_supported(n: int, k: int) -> bool:
    return int(load().g2048_mlp_fwd_lds_bytes(n, k)) > 0


def mlp_fwd(x, w, gamma, beta, residual: bool, g, y, mean, rstd, drop: Dropout | None = None):
    """g = x w^T; y = [x +] Dropout(ReLU(LayerNorm(g))) in one MFMA kernel (bf16 x [m,k], w [n,k])."""
    m, k = x.shape
    n = w.shape[0]
    _call("g2048_mlp_fwd", _stream(x), _dev(x, torch.bfloat16, "x"), _dev(w, torch.bfloat16, "w"),
          _dev(gamma, torch.float32, "gamma"), _dev(beta, torch.float32, "beta"), int(bool(residual)),
          _dev(g, torch.bfloat16, "g"), _dev(y, torch.bfloat16, "y"), _dev(mean, torch.float32, "mean"),
          _dev(rstd, torch.float32, "rstd"), m, n, k, ctypes.byref(drop) if drop is not None else None)


def head_fwd(x, wa, ba, wv, bv, logits, value):
    """logits [m, >=4] (row stride may exceed 4) and value [m] of the GameMLP heads on MFMA."""
    m, h = x.shape
    if logits.stride(-1) != 1 or logits.dtype != torch.float32 or not logits.is_cuda:
        raise G2048Error("logits must be a float32 device tensor with unit inner stride")
    _call("g2048_head_fwd", _stream(x), _dev(x, torch.bfloat16, "x"), _dev(wa, torch.float32, "wa"),
          _dev(ba, torch.float32, "ba"), _dev(wv, torch.float32, "wv"), _dev(bv, torch.float32, "bv"), m, h,
          ctypes.c_void_p(logits.data_ptr()), logits.stride(0), _dev(value, torch.float32, "value"))


def linear_dgrad_supported(n: int, k: int) -> bool:
    return bool(load().g2048_linear_dgrad_supported(int(n), int(k)))


def linear_dgrad(dg, w, out):
    """out = dg @ w on bf16 MFMA (dg [m, n], w [n, k] the Linear weight, out [m, k], all bf16)."""
    m, n = dg.shape
    k = w.shape[1]
    if w.shape[0] != n or out.shape != (m, k):
        raise G2048Error("linear_dgrad: shape mismatch")
    _call("g2048_linear_dgrad", _stream(dg), _dev(dg, torch.bfloat16, "dg"), _dev(w, torch.bfloat16, "w"),
          _dev(out, torch.bfloat16, "out"), m, n, k)


def policy_rollout_supported(hidden: int, num_layers: int) -> bool:
    return bool(load().g2048_policy_rollout_supported(int(hidden), int(num_layers)))


def policy_rollout(buf, t0: int, t1: int, w_stem, w_block, ln_gamma, ln_beta, head_bf16, ba, bv, seed: int,
                   env_base: int, counter_dev, opts: int, counter: int = 0, debug=None):
    """Steps t0 .. t1-1 of a rollout buffer (g2048/rollout.RolloutBuffers) in one fused launch:
    GameMLP (bf16 weights w_stem [h,48], w_block[2] [h,h]; fp32 LayerNorm affines; bf16 heads
    head_bf16 [5, 32*ceil(h/32)]) + sampler + env step, records bitwise the per-step path's."""
    n = buf.boards.shape[1]
    h = w_stem.shape[0]
    T = buf.actions.shape[0]
    if not (0 <= t0 <= t1 <= T) or len(w_block) != 2 or len(ln_gamma) != 3 or len(ln_beta) != 3:
        raise G2048Error("policy_rollout: bad step range or layer count")
    a = PolicyRolloutArgs()
    a.boards = _dev(buf.boards, torch.int8, "boards")
    a.flags = _dev(buf.flags, torch.uint8, "flags")
    a.actions = _dev(buf.actions, torch.uint8, "actions")
    a.logp = _dev(buf.logp, torch.float32, "logp")
    a.entropy = _dev(buf.entropy, torch.float32, "entropy")
    a.value = _dev(buf.value, torch.float32, "value")
    a.points = _dev(buf.points, torch.int32, "points")
    a.max_tile = _dev(buf.max_tile, torch.int8, "max_tile")
    a.pot = _dev(buf.pot, torch.int8, "pot")
    a.n, a.t0, a.t1, a.hidden, a.num_layers = n, t0, t1, h, len(w_block)
    a.opts, a.env_base = opts, env_base
    a.w_stem = _dev(w_stem, torch.bfloat16, "w_stem")
    for i, w in enumerate(w_block):
        a.w_block[i] = _dev(w, torch.bfloat16, "w_block")
    for i in range(3):
        a.ln_gamma[i] = _dev(ln_gamma[i], torch.float32, "ln_gamma")
        a.ln_beta[i] = _dev(ln_beta[i], torch.float32, "ln_beta")
    a.head_bf16 = _dev(head_bf16, torch.bfloat16, "head_bf16")
    a.head_bias_action = _dev(ba, torch.float32, "ba")
    a.head_bias_value = _dev(bv, torch.float32, "bv")
    a.seed, a.counter = seed & (2**64 - 1), counter
    a.counter_dev = _dev(counter_dev, torch.int64, "counter_dev")
    a.debug = _dev(debug, torch.float32, "debug")
    _call("g2048_policy_rollout", _stream(buf.boards), ctypes.byref(a))


def ppo_stats(sums, kl, grad_norm, beta_dev, critic: float, m: int, stats, counter=None, kl_rows: int = 0, rows=None):
    """kl: final {sum, max}, or (kl_rows > 0) the partial rows of a deferred ppo_head_kl."""
    _call("g2048_ppo_stats", _stream(stats), _dev(sums, torch.float32, "sums"), _dev(kl, torch.float32, "kl"),
          int(kl_rows), _dev(grad_norm, torch.float32, "grad_norm"), _dev(beta_dev, torch.float32, "beta"),
          float(critic), int(m), _dev(rows, torch.int64, "rows"), _dev(stats, torch.float32, "stats"),
          _dev(counter, torch.int64, "counter"))


# ---------------------------------------------------------------- GameURM (include/g2048_urm.h) ----
def urm_stem(obs, w, ln_w, ln_b, init_hidden, emb, x, xb):
    """emb = SiLU(LayerNorm(obs-cell features W^T)); x = init_hidden + emb; xb = bf16(x)."""
    n = obs.shape[0]
    h = w.shape[0]
    if obs.dtype not in (torch.float32, torch.bfloat16):
        raise G2048Error("obs must be float32 or bfloat16")
    _call("g2048_urm_stem", _stream(obs), _dev(obs, None, "obs"), int(obs.dtype == torch.bfloat16),
          _dev(w, torch.float32, "w"), _dev(ln_w, torch.float32, "ln_w"), _dev(ln_b, torch.float32, "ln_b"),
          _dev(init_hidden, torch.float32, "init_hidden"), _dev(emb, torch.float32, "emb"), _dev(x, torch.float32, "x"),
          _dev(xb, torch.bfloat16, "xb"), n, h)


def urm_attention(qkv, out, heads: int, p: float = 0.0, seed: int = 0, counter=None, offset: int = 0):
    """counter: device int64 [1] call counter of the dropout mask (required when p > 0); the mask is
    keyed by *counter + offset."""
    rows, h3 = qkv.shape
    if p > 0.0:
        _call("g2048_urm_attention_drop_at", _stream(qkv), _dev(qkv, torch.bfloat16, "qkv"),
              _dev(out, torch.bfloat16, "out"), rows // 16, h3 // 3, int(heads), float(p), int(seed) & (2 ** 64 - 1),
              _dev(counter, torch.int64, "counter"), int(offset))
        return
    _call("g2048_urm_attention", _stream(qkv), _dev(qkv, torch.bfloat16, "qkv"), _dev(out, torch.bfloat16, "out"),
          rows // 16, h3 // 3, int(heads))


def urm_attention_bwd(qkv, dout, dqkv, heads: int, p: float = 0.0, seed: int = 0, counter=None, offset: int = 0):
    rows, h3 = qkv.shape
    if p > 0.0:
        _call("g2048_urm_attention_bwd_drop_at", _stream(qkv), _dev(qkv, torch.bfloat16, "qkv"),
              _dev(dout, torch.bfloat16, "dout"), _dev(dqkv, torch.bfloat16, "dqkv"), rows // 16, h3 // 3, int(heads),
              float(p), int(seed) & (2 ** 64 - 1), _dev(counter, torch.int64, "counter"), int(offset))
        return
    _call("g2048_urm_attention_bwd", _stream(qkv), _dev(qkv, torch.bfloat16, "qkv"), _dev(dout, torch.bfloat16, "dout"),
          _dev(dqkv, torch.bfloat16, "dqkv"), rows // 16, h3 // 3, int(heads))


def urm_stem_partials(n: int) -> int:
    return int(load().g2048_urm_stem_partials(n))


def _obs_dtype(obs) -> int:
    if obs.dtype not in (torch.float32, torch.bfloat16):
        raise G2048Error(f"obs must be float32 or bfloat16, got {obs.dtype}")
    return 1 if obs.dtype == torch.bfloat16 else 0


def urm_stem_fwd(obs, w, ln_w, ln_b, emb, eps: float):
    rows, h = emb.shape
    _call("g2048_urm_stem_fwd", _stream(obs), _dev(obs, None, "obs"), _obs_dtype(obs), _dev(w, torch.float32, "w"),
          _dev(ln_w, torch.float32, "ln_w"), _dev(ln_b, torch.float32, "ln_b"), _dev(emb, torch.float32, "emb"),
          rows // 16, h, float(eps))


def urm_stem_bwd(obs, w, ln_w, ln_b, demb, grads, partials, eps: float):
    rows, h = demb.shape
    _call("g2048_urm_stem_bwd", _stream(obs), _dev(obs, None, "obs"), _obs_dtype(obs), _dev(w, torch.float32, "w"),
          _dev(ln_w, torch.float32, "ln_w"), _dev(ln_b, torch.float32, "ln_b"), _dev(demb, torch.float32, "demb"),
          _dev(grads, torch.float32, "grads"), _dev(partials, torch.float32, "partials"), rows // 16, h, float(eps))


def urm_stem_bwd3(obs, w, ln_w, ln_b, demb, dw, dln_w, dln_b, partials, eps: float, accumulate: bool = False):
    """g2048_urm_stem_bwd3: the three stem gradients at their own addresses (accumulate: added to)."""
    rows, h = demb.shape
    _call("g2048_urm_stem_bwd3", _stream(obs), _dev(obs, None, "obs"), _obs_dtype(obs), _dev(w, torch.float32, "w"),
          _dev(ln_w, torch.float32, "ln_w"), _dev(ln_b, torch.float32, "ln_b"), _dev(demb, torch.float32, "demb"),
          _dev(dw, torch.float32, "dw"), _dev(dln_w, torch.float32, "dln_w"), _dev(dln_b, torch.float32, "dln_b"),
          int(bool(accumulate)), _dev(partials, torch.float32, "partials"), rows // 16, h, float(eps))


def urm_rms_res_fwd(h, a, out, rstd, eps: float, outb=None):
    """outb: optional bf16 [rows, 64] copy of out (g2048_urm_rms_res_fwd2)."""
    rows, hid = h.shape
    abf = a.dtype == torch.bfloat16
    _call("g2048_urm_rms_res_fwd2", _stream(h), _dev(h, torch.float32, "h"),
          _dev(a, torch.bfloat16 if abf else torch.float32, "a"), int(abf), _dev(out, torch.float32, "out"),
          _dev(outb, torch.bfloat16, "outb"), _dev(rstd, torch.float32, "rstd"), rows, hid, float(eps))


def urm_add_cast(a, a_rows: int, e, out, outb):
    """out = a + e, outb = bf16(out) (g2048_urm_add_cast); a broadcast over groups of a_rows rows
    when a_rows > 0."""
    rows, hid = e.shape
    _call("g2048_urm_add_cast", _stream(e), _dev(a, torch.float32, "a"), int(a_rows), _dev(e, torch.float32, "e"),
          _dev(out, torch.float32, "out"), _dev(outb, torch.bfloat16, "outb"), rows, hid)


def urm_add_cast_bwd(dout, doutb, dx, acc_in=None, acc_out=None):
    """dx = dout + float(doutb) (either may be None); acc_out = acc_in + dx when given, dx may then be
    None (g2048_urm_add_cast_bwd_acc)."""
    ref = dx if dx is not None else acc_out
    rows, hid = ref.shape
    _call("g2048_urm_add_cast_bwd_acc", _stream(ref), _dev(dout, torch.float32, "dout"),
          _dev(doutb, torch.bfloat16, "doutb"), _dev(dx, torch.float32, "dx"), _dev(acc_in, torch.float32, "acc_in"),
          _dev(acc_out, torch.float32, "acc_out"), rows, hid)


def urm_rms_res_bwd(dout, out, rstd, dh, da, doutb=None, dpool=None):
    """dout fp32 and / or doutb bf16 (the bf16 copy's gradient); either may be None.  dpool (instead of
    dout): fp32 [rows / 16, 64] broadcast over each board's 16 token rows (the mean-pool backward)."""
    rows, hid = out.shape
    abf = da.dtype == torch.bfloat16
    _call("g2048_urm_rms_res_bwd3", _stream(out), _dev(dout, torch.float32, "dout"),
          _dev(dpool, torch.float32, "dpool"), _dev(doutb, torch.bfloat16, "doutb"), _dev(out, torch.float32, "out"),
          _dev(rstd, torch.float32, "rstd"), _dev(dh, torch.float32, "dh"),
          _dev(da, torch.bfloat16 if abf else torch.float32, "da"), int(abf), rows, hid)


def urm_swiglu_conv_partials(n: int, inter: int) -> int:
    return int(load().g2048_urm_swiglu_conv_partials(n, inter))


def urm_gate_up_swiglu_bwd_supported(h: int, inter: int) -> bool:
    return bool(load().g2048_urm_gate_up_swiglu_bwd_supported(h, inter))


def urm_gate_up_swiglu_bwd(x, w, conv_w, conv_b, dact, dgu, dw, db, partials, accumulate: bool = False):
    """dgu, dw, db of the SwiGLU-conv with gu = bf16(x w^T) recomputed on MFMA
    (g2048_urm_gate_up_swiglu_bwd_acc; accumulate: dw / db += the sums)."""
    rows, h = x.shape
    inter = w.shape[0] // 2
    _call("g2048_urm_gate_up_swiglu_bwd_acc", _stream(x), _dev(x, torch.bfloat16, "x"), _dev(w, torch.bfloat16, "w"),
          _dev(conv_w, torch.float32, "conv_w"), _dev(conv_b, torch.float32, "conv_b"),
          _dev(dact, torch.bfloat16, "dact"), _dev(dgu, torch.bfloat16, "dgu"), _dev(dw, torch.float32, "dw"),
          _dev(db, torch.float32, "db"), _dev(partials, torch.float32, "partials"), rows // 16, h, inter,
          int(bool(accumulate)))


def urm_swiglu_conv_fwd(gu, w, b, act):
    rows, inter = act.shape
    _call("g2048_urm_swiglu_conv_fwd", _stream(gu), _dev(gu, torch.bfloat16, "gu"), _dev(w, torch.float32, "w"),
          _dev(b, torch.float32, "b"), _dev(act, torch.bfloat16, "act"), rows // 16, inter)


def urm_swiglu_conv_bwd(gu, w, b, dact, dgu, dw, db, partials):
    rows, inter = dact.shape
    _call("g2048_urm_swiglu_conv_bwd", _stream(gu), _dev(gu, torch.bfloat16, "gu"), _dev(w, torch.float32, "w"),
          _dev(b, torch.float32, "b"), _dev(dact, torch.bfloat16, "dact"), _dev(dgu, torch.bfloat16, "dgu"),
          _dev(dw, torch.float32, "dw"), _dev(db, torch.float32, "db"), _dev(partials, torch.float32, "partials"),
          rows // 16, inter)


def urm_residual_rms(x, y, emb, xb, eps: float):
    rows, h = x.shape
    _call("g2048_urm_residual_rms", _stream(x), _dev(x, torch.float32, "x"), _dev(y, torch.bfloat16, "y"),
          _dev(emb, torch.float32, "emb"), _dev(xb, torch.bfloat16, "xb"), rows, h, float(eps))


def urm_swiglu_conv(gu, w, b, out):
    rows, inter2 = gu.shape
    _call("g2048_urm_swiglu_conv", _stream(gu), _dev(gu, torch.bfloat16, "gu"), _dev(w, torch.float32, "w"),
          _dev(b, torch.float32, "b"), _dev(out, torch.bfloat16, "out"), rows // 16, inter2 // 2)


def urm_pool_heads(x, wa, ba, wv, bv, logits, value):
    rows, h = x.shape
    _call("g2048_urm_pool_heads", _stream(x), _dev(x, torch.float32, "x"), _dev(wa, torch.float32, "wa"),
          _dev(ba, torch.float32, "ba"), _dev(wv, torch.float32, "wv"), _dev(bv, torch.float32, "bv"),
          _dev(logits, torch.float32, "logits"), _dev(value, torch.float32, "value"), rows // 16, h)


def urm_linear_supported(epilogue: int, k: int, n: int, inter: int = 0) -> bool:
    return bool(load().g2048_urm_linear_supported(int(epilogue), int(k), int(n), int(inter)))


def urm_linear(inp, w, out):
    """out = inp w^T (bf16, fp32 accumulate) on the fused-projection kernel (qkv_proj)."""
    rows, k = inp.shape
    _call("g2048_urm_linear", _stream(inp), _dev(inp, torch.bfloat16, "in"), _dev(w, torch.bfloat16, "w"),
          _dev(out, torch.bfloat16, "out"), rows, k, w.shape[0])


def urm_linear_t(inp, w, out):
    """out = inp w for w [k, n] (bf16): dX = dY W without a transposed copy (g2048_urm_linear_t)."""
    rows, k = inp.shape
    _call("g2048_urm_linear_t", _stream(inp), _dev(inp, torch.bfloat16, "in"), _dev(w, torch.bfloat16, "w"),
          _dev(out, torch.bfloat16, "out"), rows, k, w.shape[1])


def urm_linear_bias(inp, w, bias, out):
    """out = bf16(inp w^T + bias) with one rounding (autocast's biased Linear; g2048_urm_linear_bias)."""
    rows, k = inp.shape
    _call("g2048_urm_linear_bias", _stream(inp), _dev(inp, torch.bfloat16, "in"), _dev(w, torch.bfloat16, "w"),
          _dev(bias, torch.float32, "bias"), _dev(out, torch.bfloat16, "out"), rows, k, w.shape[0])


def urm_linear_res_rms(inp, w, h, out, outb, rstd, eps: float):
    """out = rms_norm(h + bf16(inp w^T)), outb = bf16(out) (optional), rstd (g2048_urm_linear_res_rms)."""
    rows, k = inp.shape
    _call("g2048_urm_linear_res_rms", _stream(inp), _dev(inp, torch.bfloat16, "in"), _dev(w, torch.bfloat16, "w"),
          _dev(h, torch.float32, "h"), _dev(out, torch.float32, "out"), _dev(outb, torch.bfloat16, "outb"),
          _dev(rstd, torch.float32, "rstd"), rows, k, w.shape[0], float(eps))


def urm_linear_rms(inp, w, x, emb, xb, eps: float):
    """x = rms_norm(x + inp w^T) [+ emb]; xb = bf16(x)  (o_proj / down_proj with the post-norm)."""
    rows, k = inp.shape
    _call("g2048_urm_linear_rms", _stream(inp), _dev(inp, torch.bfloat16, "in"), _dev(w, torch.bfloat16, "w"),
          _dev(x, torch.float32, "x"), _dev(emb, torch.float32, "emb"), _dev(xb, torch.bfloat16, "xb"), rows, k,
          w.shape[0], float(eps))


def urm_wgrad_supported(n: int, k: int) -> bool:
    """g2048_urm_wgrad covers dw [n, k] (the projection shapes of the URM training Functions)."""
    return bool(load().g2048_urm_wgrad_supported(n, k))


def urm_wgrad_partials(m: int, n: int, k: int) -> int:
    return int(load().g2048_urm_wgrad_partials(m, n, k))


def lds_poison(word: int, device=None):
    """Test hook: every CU's LDS filled with the 32-bit `word` (g2048_lds_poison)."""
    dev = device or torch.device("cuda", torch.cuda.current_device())
    _call("g2048_lds_poison", ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), int(word) & 0xFFFFFFFF)


def urm_head_loss_partials(m: int, h: int) -> int:
    return int(load().g2048_urm_head_loss_partials(m, h))


def _pooled_dtype(t) -> int:
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise G2048Error("pooled must be float32 or bfloat16")
    return int(t.dtype == torch.bfloat16)


def urm_head_loss(pooled, wa, ba, wv, bv, batch: PPOBatch, beta_dev, critic, clip_eps, dz, masked, partials, sync,
                  sums, loss):
    """GameURM's heads + PPO loss + dz / masked / sums / loss (g2048_urm_head_loss)."""
    m, h = pooled.shape
    _call("g2048_urm_head_loss", _stream(pooled), _dev(pooled, None, "pooled"), _pooled_dtype(pooled),
          _dev(wa, torch.float32, "wa"), _dev(ba, torch.float32, "ba"), _dev(wv, torch.float32, "wv"),
          _dev(bv, torch.float32, "bv"), m, h, ctypes.byref(batch), _dev(beta_dev, torch.float32, "beta"),
          float(critic), float(clip_eps), _dev(dz, torch.float32, "dz"), _dev(masked, torch.float32, "masked"),
          _dev(partials, torch.float32, "partials"), _dev(sync, torch.int32, "sync"), _dev(sums, torch.float32, "sums"),
          _dev(loss, torch.float32, "loss"))


def urm_head_loss_bwd(pooled, wa, wv, dz, grad_out, dpooled, partials, sync, dwa, dba, dwv, dbv,
                      accumulate: bool = False):
    """dpooled and the head gradients of g2048_urm_head_loss (g2048_urm_head_loss_bwd)."""
    m, h = pooled.shape
    _call("g2048_urm_head_loss_bwd", _stream(pooled), _dev(pooled, None, "pooled"), _pooled_dtype(pooled),
          _dev(wa, torch.float32, "wa"), _dev(wv, torch.float32, "wv"), _dev(dz, torch.float32, "dz"),
          _dev(grad_out, torch.float32, "grad_out"), _dev(dpooled, pooled.dtype, "dpooled"),
          _dev(partials, torch.float32, "partials"), _dev(sync, torch.int32, "sync"), _dev(dwa, torch.float32, "dwa"),
          _dev(dba, torch.float32, "dba"), _dev(dwv, torch.float32, "dwv"), _dev(dbv, torch.float32, "dbv"),
          int(bool(accumulate)), m, h)


def urm_kl_stats(old_masked, logits, sums, gn, beta_dev, critic, stats, partials, sync):
    """KL(old || new) + the minibatch statistics update (g2048_urm_kl_stats)."""
    _call("g2048_urm_kl_stats", _stream(logits), _dev(old_masked, torch.float32, "old_masked"),
          _dev(logits, torch.float32, "logits"), logits.shape[0], _dev(sums, torch.float32, "sums"),
          _dev(gn, torch.float32, "gn"), _dev(beta_dev, torch.float32, "beta"), float(critic),
          _dev(stats, torch.float32, "stats"), _dev(partials, torch.float32, "partials"),
          _dev(sync, torch.int32, "sync"))


def urm_wgrad(dy, x, dw, partials, accumulate: bool = False):
    """dw fp32 [n, k] = dy^T x (g2048_urm_wgrad_acc; accumulate: dw += dy^T x); dy bf16 [m, n], x bf16 [m, k]."""
    m, n = dy.shape
    _call("g2048_urm_wgrad_acc", _stream(dy), _dev(dy, torch.bfloat16, "dy"), _dev(x, torch.bfloat16, "x"),
          _dev(dw, torch.float32, "dw"), _dev(partials, torch.float32, "partials"), m, n, x.shape[1],
          int(bool(accumulate)))


def urm_linres_bwd_supported(hidden: int, k: int) -> bool:
    return bool(load().g2048_urm_linres_bwd_supported(hidden, k))


def urm_linres_bwd_partials(rows: int, k: int) -> int:
    return int(load().g2048_urm_linres_bwd_partials(rows, k))


def urm_linres_bwd(out, rstd, w, x, dh, dw, partials, dout=None, dpool=None, doutb=None, dx=None,
                   accumulate: bool = False):
    """The residual-RMSNorm projection's backward in one pass (g2048_urm_linres_bwd): dh fp32 [rows, 64],
    dx bf16 [rows, k] (None: skipped), dw fp32 [64, k] (+= with accumulate) from dout fp32 [rows, 64] /
    dpool fp32 [rows / 16, 64] / doutb bf16 [rows, 64] (each may be None), out fp32, rstd fp32 [rows],
    w bf16 [64, k], x bf16 [rows, k]."""
    rows, hid = out.shape
    k = x.shape[1]
    _call("g2048_urm_linres_bwd", _stream(out), _dev(dout, torch.float32, "dout"), _dev(dpool, torch.float32, "dpool"),
          _dev(doutb, torch.bfloat16, "doutb"), _dev(out, torch.float32, "out"), _dev(rstd, torch.float32, "rstd"),
          _dev(w, torch.bfloat16, "w"), _dev(x, torch.bfloat16, "x"), _dev(dh, torch.float32, "dh"),
          _dev(dx, torch.bfloat16, "dx"), _dev(dw, torch.float32, "dw"), _dev(partials, torch.float32, "partials"),
          int(bool(accumulate)), rows, hid, k)


def urm_linear_swiglu_train(inp, w, conv_w, conv_b, gu, act):
    rows, h = inp.shape
    _call("g2048_urm_linear_swiglu_train", _stream(inp), _dev(inp, torch.bfloat16, "in"), _dev(w, torch.bfloat16, "w"),
          _dev(conv_w, torch.float32, "conv_w"), _dev(conv_b, torch.float32, "conv_b"), _dev(gu, torch.bfloat16, "gu"),
          _dev(act, torch.bfloat16, "act"), rows, h, act.shape[1])


def urm_linear_swiglu(inp, w, conv_w, conv_b, out):
    """out = SiLU(dwconv(SiLU(gate) * up)) with [gate | up] = inp w^T (gate_up_proj + ConvSwiGLU)."""
    rows, h = inp.shape
    _call("g2048_urm_linear_swiglu", _stream(inp), _dev(inp, torch.bfloat16, "in"), _dev(w, torch.bfloat16, "w"),
          _dev(conv_w, torch.float32, "conv_w"), _dev(conv_b, torch.float32, "conv_b"),
          _dev(out, torch.bfloat16, "out"), rows, h, w.shape[0] // 2)


def urm_forward_supported(hidden: int, heads: int, inter: int, num_layers: int, conv_kernel: int) -> bool:
    return bool(load().g2048_urm_forward_supported(int(hidden), int(heads), int(inter), int(num_layers),
                                                   int(conv_kernel)))


def urm_forward_drop(weights: UrmWeights, obs, logits, value, p: float, seed: int, counter):
    """g2048_urm_forward in training mode (attention dropout p, mask counter *counter + block app)."""
    if obs.dtype not in (torch.float32, torch.bfloat16):
        raise G2048Error("obs must be float32 or bfloat16")
    _call("g2048_urm_forward_drop", _stream(obs), ctypes.byref(weights), _dev(obs, None, "obs"),
          int(obs.dtype == torch.bfloat16), _dev(logits, torch.float32, "logits"), _dev(value, torch.float32, "value"),
          obs.shape[0], float(p), int(seed) & (2 ** 64 - 1), _dev(counter, torch.int64, "counter"))


def urm_forward(weights: UrmWeights, obs, logits, value):
    """The whole GameURM forward in one launch (g2048_urm_forward); `weights` holds device pointers."""
    if obs.dtype not in (torch.float32, torch.bfloat16):
        raise G2048Error("obs must be float32 or bfloat16")
    _call("g2048_urm_forward", _stream(obs), ctypes.byref(weights), _dev(obs, None, "obs"),
          int(obs.dtype == torch.bfloat16), _dev(logits, torch.float32, "logits"), _dev(value, torch.float32, "value"),
          obs.shape[0])
