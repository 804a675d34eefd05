/*
 * g2048_ntuple.h -- n-tuple network with afterstate TD(0) learning (Szubert & Jaskowski 2014; Yeh et
 * al. 2016), optionally with temporal-coherence step sizes, on the 2048 engine of g2048.h: the
 * table-based learner a 2048 agent is compared with.  No reference counterpart.  The conventions are
 * those of g2048.h: device pointers (except the host structs g2048_ntuple_net / g2048_rng, read during
 * the call), asynchronous on `stream`, no allocation and no host synchronisation (hipGraph-capturable),
 * 0 / G2048_EINVAL (nothing enqueued) / a positive hipError_t, n = 0 a no-op.  This text is the
 * specification; tests/ntuple_reference.py restates it, tests/ntuple_tc_reference.py the TC step,
 * tests/ntuple_lambda_reference.py the lambda step, tests/ntuple_stage_reference.py the stages,
 * tests/ntuple_carousel_reference.py the carousel.
 *
 * The network.  T tuples of K cells each (cell = 4 row + col) and one table of 16^K int32 weights per
 * tuple.  All values are integers: points x S, S = 2^G2048_NT_FRAC_BITS = 4096.
 *   e(b, c)  = min(b[c], 15)                                   the exponent of cell c, clamped
 *   idx_t(b) = sum over j < K of e(b, cells[K t + j]) << 4 j
 *   V(b)     = sum over t < T and over the 8 symmetries g of the square of W_t[idx_t(g(b))]   (int64)
 * The sum runs over the whole symmetry group (4 rotations x an optional reflection), so it does not
 * depend on how the eight are enumerated, and V(g(b)) = V(b).  A tuple that a symmetry maps onto
 * itself reads one weight twice: that is intended, in the value and in the update.
 *
 * The choice.  move(b, a), its merge points pts(b, a) and legality (move(b, a) != b) are
 * g2048_env_step's; move(b, a) is the after-state: moved, before the spawn.
 *   q[a] = S pts(b, a) + V(move(b, a)) for a legal a, INT64_MIN for an illegal a
 *   best = the legal action of the largest q, the lowest index among equals, 0xFF without a legal move
 *   legal = bits 0-3 the legal actions (the conventions of g2048_mc_search)
 *
 * The TD step.  Env i at step t < steps uses Philox counter c + t, c = rng->counter (+ *counter_dev).
 * Every read of a step sees the weights as they were before that step's updates.
 *   1. the greedy action of boards[i]: with a legal move a* = best, target = q[a*], s' = move(board, a*);
 *      without one there is no move and target = 0.
 *   2. if pending[i] != 0:  delta = (pending[i] == 2 ? 0 : target) - V(after[i])
 *        D = clamp((delta + (1 << (lr_shift - 1))) >> lr_shift, -2^30, 2^30)     arithmetic shift
 *      and D is added to each of the 8 T weights (counted with multiplicity) that V(after[i]) reads.
 *      Such an (env, step) counts as one update applied, whatever D is.
 *   3. the env is stepped: exactly g2048_env_step with the action a* (0 without a legal move) and
 *      G2048_OPT_AUTO_RESET at counter c + t, env id rng->env_base + i.  run_score[i] += points; on
 *      G2048_FLAG_DONE the finished score run_score[i] goes into stats and run_score[i] = 0.
 *   4. with a legal move after[i] = s' and pending[i] = DONE ? 2 : 1; without one pending[i] = 0.
 * So pending[i] = 0: no after-state is waiting (the start: zero-fill it); 1: after[i] waits for the
 * value of the next board; 2: after[i] ended its game, its target is 0.
 * Updates are integer adds, which commute: the weights after a step do not depend on the order in
 * which the n envs add, and a run is bitwise reproducible.
 * Range.  The weights WRAP on overflow (two's complement): one weight holds +-2^31 / S = +-2^19
 * points.  Concurrent envs add up on shared weights, so a usable lr_shift grows with n: from zero
 * weights, five 4-tuples and n = 256, lr_shift 9 drove weights to 2^31 while lr_shift 10 learned.
 *
 * The TC step (g2048_ntuple_tc): temporal-coherence learning (Beal & Smith 1999; Jaskowski 2018), a step
 * size per weight instead of the one lr_shift.  Every weight i of the net has an accumulator record
 * of 16 bytes in the device array tc, int64 [T][16^K][2]: tc[2 i] = E_i, the sum of the D it received
 * (int64), tc[2 i + 1] = A_i, the sum of their |D| (read as uint64).  Both wrap like the weights;
 * zero-filled means "never updated".  A weight moves at the rate |E_i| / A_i: one whose errors agree
 * keeps learning at the full rate, one whose errors cancel slows itself down.
 * A TC step is the TD step, 1-4, with step 2 replaced: delta and D are computed exactly as there, and
 * for each of the 8 T weights i that V(after[i]) reads, counted with multiplicity, with E_i and A_i as
 * they were before this step's adds,
 *   A_i == 0:  add_i = D
 *   otherwise: sh = max(bitlen(A_i) - 20, 0),  a = A_i >> sh  (1 <= a < 2^20),
 *              e = min(|E_i| >> sh, a)         |E_i| the unsigned magnitude: 2^63 for INT64_MIN
 *              add_i = sign(D) floor((|D| e + (a >> 1)) / a)
 *   W_i += add_i (int32, wraps),  E_i += D,  A_i += |D|.
 * Every read of a step (W, E, A) sees the values before that step's adds: the read-before-write rule
 * of the TD step, extended to the accumulators.  A self-symmetric tuple hits one weight twice: both
 * hits read the same record, and W, E and A each receive two adds.  An (env, step) with pending != 0
 * counts as one update applied, as there.  |D| <= 2^30 and e < 2^20, so the numerator is below 2^51 and
 * the quotient at most |D|; the integer result is the specification, however it is divided.  The min
 * makes the rule total on any accumulator contents; in a run from zeros |E| <= A holds without it.
 * With D = 0 nothing changes: no weight, no E, no A.  With every A = 0 the first hit of every weight is
 * plain TD(0): lr_shift is the base rate at which a fresh weight starts.  All adds are integer adds of
 * values fixed by the reads, so they commute and a run stays bitwise reproducible.
 *
 * The lambda step (g2048_ntuple_lambda): TD(lambda) and TC(lambda) with a truncated eligibility trace
 * (Yeh et al. 2016; Jaskowski 2018) and lambda = 2^-s, s = lambda_shift in 1..G2048_NT_MAX_LAMBDA_SHIFT,
 * so that the decay is a shift and every update stays an integer add.  The error of after[i] is also
 * passed back to the h = trace_len <= G2048_NT_MAX_TRACE after-states before it in the same game.
 * Carried beside after / pending:
 *   hist      int8 [h][n][16] (device, 16-B aligned): hist[k][i] is the after-state of env i that is
 *             k + 1 moves older than after[i], in the same game
 *   hist_len  uint8 [n]: how many of them are valid, 0..h; zero-filled at the start
 * The lambda step is the TD step 1-4 with steps 2 and 4 extended; p = pending[i] as read at the start
 * of the step.  Steps 1 and 3 are unchanged.
 *   2. if p != 0: delta and D exactly as in the TD step (the same rounding shift by lr_shift, the same
 *      clamp to +-2^30).  For k = 0 .. hist_len[i]:
 *        D_k = sign(D) (|D| >> k s)          D_0 = D; the decay rounds towards zero, symmetrically
 *        s_0 = after[i],  s_k = hist[k - 1][i]
 *      and for every k with D_k != 0 the update of the chosen rule is applied to each of the 8 T weights
 *      that V(s_k) reads, counted with multiplicity, with D_k in the place of D:
 *        rule TD:  W += D_k
 *        rule TC:  add_i, E_i += D_k and A_i += |D_k| exactly as the TC step defines them
 *      One weight may be hit from several k and several envs in one step: all those hits read W, E and
 *      A as they were before this step's adds.  Such an (env, step) still counts as one update applied.
 *   4. with a legal move and p == 1: hist[k][i] = hist[k - 1][i] for k = h - 1 .. 1, hist[0][i] = the old
 *      after[i], hist_len[i] = min(hist_len[i] + 1, h).  With a legal move and p != 1 (nothing was
 *      waiting, or after[i] ended its game), and without a legal move: hist_len[i] = 0.  Then after /
 *      pending are set as in the TD step.
 * So a terminal update (p == 2, target 0) still reaches the history of the game that ended, and the
 * first after-state of the next game starts with an empty history.  Rows of hist at or beyond
 * hist_len[i] hold nothing: they are neither used nor kept.
 * Bounds.  k s <= 4 x 7 = 28, so the shift is always defined; |D_k| <= |D| <= 2^30, so the TC numerator
 * bound holds unchanged.  With h = 0 the lambda step is the TD step (or the TC step) bit for bit.  The
 * adds are still integer adds of values fixed by the reads: a run stays bitwise reproducible.
 * Range.  A trace adds up to 1 + 2^-s + .. + 2^-hs of D to weights that consecutive after-states share,
 * so under rule TD a usable lr_shift grows with h as it grows with n: from zero weights, five 4-tuples,
 * n = 256, h = 3 and s = 1, lr_shift 10 collapsed (mean score near 1 000) while lr_shift 11 learned; rule
 * TC learned at lr_shift 10 with and without the trace.
 *
 * The search (g2048_ntuple_search).  Expectimax with V at the leaves: d = depth in 1..3 moves looked
 * ahead, the root move included; E(s) = the number of empty cells of s; s + t@c = s with exponent t
 * put on its empty cell c.  All values are int64 in points x S.
 *   A(s, 0) = V(s)                                                  leaf: an after-state
 *   A(s, k) = floor( sum over the empty cells c of s of (9 M(s + 1@c, k) + M(s + 2@c, k)) / (10 E(s)) ),  k >= 1
 *   M(b, k) = max over the legal a of (S pts(b, a) + A(move(b, a), k - 1));   0 without a legal move
 *   q[i][a] = S pts(root_i, a) + A(move(root_i, a), d - 1) for a legal a,  INT64_MIN for an illegal a
 *   best    = the legal action of the largest q, the lowest index among equals, 0xFF without a legal move
 *   legal   = bits 0-3, the conventions of g2048_ntuple_choose
 *   leaves[i][a] = the number of A(., 0) evaluations under root action a, 0 for an illegal one
 * At d = 1 this is g2048_ntuple_choose bit for bit.  Three points differ from g2048_expectimax:
 * Values are signed.  Weights are any int32, so V, M and the chance sums can be negative.  floor is the
 * floor towards minus infinity (Python's //), not C's truncating /.  Illegal actions are marked
 * INT64_MIN, as in g2048_ntuple_choose, because -1 is a valid value here.  The maximum over the legal
 * moves starts from "none": only a board without a legal move yields 0, the terminal target of the TD
 * step -- so a dead position can be better than a live one of negative value; that is intended.
 * The sum inside A is exact before its one division: no result depends on summation order or on the
 * lane mapping (`form`).
 * Bound.  |V| <= 64 x 2^31 = 2^37; S pts < 2^31 per ply, so |M| < 2^38 for d <= 3; a chance node sums at
 * most 160 weighted terms, |sum| < 2^46.  The signed floor is the unsigned one of sum + 10 E 2^40
 * (< 2^48), minus 2^40: exact.  Depth 4 is out of scope.
 *
 * Stages (Yeh et al. 2016; Jaskowski 2018).  A game is not stationary: one pattern means different things
 * on a board whose largest tile is 256 and on one that holds a 2048.  A staged net keeps one set of
 * tables per stage of the game, and the stage of a board is a function of its largest tile:
 *   m(b)     = max over the 16 cells c of e(b, c)       clamped to 15 like every exponent; 0: the empty board
 *   stage(b) = nibble m(b) of stage_map                 bits 4 m .. 4 m + 3
 *   G        = 1 + nibble 15 of stage_map               the number of stages, 1..G2048_NT_MAX_STAGES
 * A map is valid when nibble 0 is 0 and every next nibble equals the one before it or is one more: the
 * stages are numbered without gaps and never decrease as the largest tile grows.  stage_map == 0 is the
 * one-stage net: every call then gives the results of the text above byte for byte.  m, and so the
 * stage, is the same for the 8 symmetric images of a board.
 * With stages, weights is int32 [G][T][16^K] and tc int64 [G][T][16^K][2], and
 *   V(b) = sum over t < T and over the 8 symmetries g of W[stage(b)][t][idx_t(g(b))].
 * "The 8 T weights that V(s) reads" are, wherever this text uses the phrase, those of stage(s): in the
 * TD update of after[i], in the records of the TC step, and for every s_k of the lambda step, each at its
 * own stage.  Nothing else changes in the choice, the three steps or the search.  In particular a target
 * q[a*] may come from another stage's tables than those of the after-state being updated: that is the
 * point of the method.  The leaves of the search evaluate V at the stage of each leaf after-state; its
 * bounds hold unchanged, since a V still sums 8 T weights.
 * Promotion (g2048_ntuple_promote) adds the tables of one stage to those of another, W[to][j] += W[from][j]
 * for every j < T 16^K, int32 and wrapping like every add on the weights: on a zero stage it is a copy, so
 * a stage can start from what the stage below it has learned instead of from nothing.  The accumulators
 * of rule TC are not touched: a promoted stage starts with "never updated" records, at the base rate.
 * The ABI.  g2048_ntuple_net and the calls that take it are unchanged: they are the one-stage net.  A net
 * with stages is a g2048_ntuple_staged_net, the same struct followed by stage_map, and every call has a
 * twin g2048_ntuple_staged_<call> that takes it and is otherwise the same call: the same arguments in the
 * same order, the same refusals (and an invalid map), the same workspace.  With stage_map == 0 a twin is
 * its one-stage call bit for bit.  C callers zero-initialise the struct (a designated initialiser does).
 *
 * Carousel (g2048_ntuple_staged_carousel; Jaskowski 2018, carousel shaping).  From the empty-board reset the
 * tables of a late stage are updated only in the last moves of the few games that get that far.  The carousel
 * remembers boards with which games entered each stage and starts finished games from them, going round the
 * stages in turn, so that every stage's tables get a comparable share of the training.  The carousel step is
 * the lambda step of a staged net with its step 3 extended; steps 1, 2 and 4, both rules and every trace_len
 * are unchanged.  G is the number of stages, c + t the Philox counter of the step.  Carried beside boards /
 * after / pending / hist, device memory, zero-filled at the start of a run and owned by the caller:
 *   pool    int8 [G][n][16] (16-B aligned): pool[g][i] is the snapshot of stage g taken by env i; row 0 is
 *           never read or written
 *   valid   uint8 [n][16] (16-B aligned): valid[i][g] != 0 means pool[g][i] holds a snapshot
 *   next    uint8 [n]: the stage at which env i's next game is to start, its place on the carousel
 *   origin  uint8 [n]: the stage the current game of env i started from; 0: the ordinary reset
 * Step 3 of the carousel step, for env i at step t:
 *   3a. the env is stepped exactly as in the TD step (the action a*, or 0 without a legal move, AUTO_RESET,
 *       counter c + t, env id env_base + i): b is the board before the step, b' the board after it, on DONE
 *       the freshly reset board.
 *   3b. not DONE and stage(b') != stage(b): the game has entered the stage g' = stage(b');
 *       pool[g'][i] = b', valid[i][g'] = 1, stats[6] += 1.
 *   3c. DONE: the game that ended is accounted.  origin[i] == 0: stats[0] += 1, stats[1] += run_score[i],
 *       stats[2] = max(stats[2], run_score[i]), as in the TD step.  Otherwise stats[4] += 1 and stats[5] +=
 *       run_score[i], the points since the restart: such a game is not a full game and stays out of the
 *       score statistics.  run_score[i] = 0.  Then the next game is chosen:
 *         j = (i + c + t) mod n     the donor slot: the sum modulo 2^64, i the local index
 *         k = next[i] if next[i] < G, else 0
 *         g = the smallest g' with max(k, 1) <= g' < G and valid[j][g'] != 0, if k >= 1 and there is one;
 *             otherwise 0
 *       g >= 1: boards[i] = pool[g][j] in place of the reset board, and stats[7] += 1; g == 0: the reset
 *       board stays.  origin[i] = g, next[i] = (g + 1) mod G.
 * Within one step the donors of the n envs are a permutation of the slots, so no two envs take the same one
 * (except in a step whose sums pass 2^64 among its n envs, for an n that does not divide 2^64: slots are only
 * read, so nothing depends on it), and the donor of an env moves on by one slot per step: the boards mix
 * between the envs without a shared buffer filled by atomics, whose contents would depend on the order of
 * arrival.
 * Every read of pool and valid in a step sees them as they were before that step's writes: the rule of the TD
 * step, extended.  next[i] is written by env i alone, so its choice is final before the step's writes.
 * What follows: a game ended by DONE still gets pending = 2 and the terminal target 0; the restarted game
 * starts with an empty trace (step 4 empties it for p != 1); with G = 1 nothing is ever recorded or restarted
 * and the call is g2048_ntuple_staged_lambda bit for bit in every carried array, the weights, tc and
 * stats[0..3]; a stage whose boards a game never enters (one the reset board is already in) is never
 * recorded, and the carousel passes over it.  A run stays bitwise reproducible.
 *
 * Optimistic initialisation (g2048_ntuple_fill, g2048_ntuple_promote_from; Guei, Chen, Wu 2021, "Optimistic
 * Temporal Difference Learning for 2048"; tests/ntuple_optimistic_reference.py).  The learner is greedy: it plays
 * the move of the largest q and never explores.  From zero tables a board never seen is worth nothing, less than
 * any board that has scored, and is never tried.  Starting every weight at one positive value turns that round:
 * every board is worth the same large V_init until the terminal target 0 and the rewards really seen pull the
 * boards a game visits down, so a board not yet visited looks better than a visited one and gets its turn.
 *   fill:  W[j] = w0 for every j < T 16^K (a staged net: every j < G T 16^K, all stages), any int32 w0.
 * Consequence: V(b) = 8 T w0 for every board b, multiplicities included (a self-symmetric tuple reads its one
 * weight twice, and both reads give w0), at every stage.  So q[a] = S pts(b, a) + 8 T w0 for every legal a: on a
 * board whose legal moves merge nothing (or the same points) they all tie, and best is the lowest legal index.
 * For V_init points the start is w0 = round(V_init S / (8 T)); the learning steps do not know of it: they run
 * from these tables exactly as from any others.  fill writes nothing outside the tables and leaves tc alone.
 * Promotion of g2048_ntuple_promote adds a whole stage, start included: onto a stage that still holds w0
 * everywhere it would leave W[from] + w0, the optimism doubled.  The promotion over a start takes it off:
 *   promote_from:  W[to][j] += W[from][j] - base  for every j < T 16^K, int32 and wrapping like every add on the
 *                  weights (the difference and the sum both modulo 2^32).
 * With base == 0 it is g2048_ntuple_promote byte for byte.  On a stage that still holds base everywhere it is a
 * copy of W[from]; on one that has learned d[j] over base it leaves base + d[j] + (W[from][j] - base): what both
 * stages learned, over one start.  The accumulators of rule TC are not touched, as in g2048_ntuple_promote.
 *
 * Tile-downgrading (g2048_ntuple_downgrade; Guei, Chen, Wu 2021; tests/ntuple_downgrade_reference.py).  A net is
 * only as good as the boards it was trained on, and the tables indexed by the largest tiles are trained last and
 * least: a player that reaches such a tile reads weights that still hold their start.  The large tiles of a board
 * are mostly a ladder, and the net knows how to play a ladder one rung lower.  So when a tile value is missing
 * below the largest tile, every tile above that gap is halved, and the player chooses its move on the translated
 * board.  It is a pure map from 16 bytes to 16 bytes; nothing of the net takes part.
 * Parameters: from_exp f in 2..31, lo_exp l in 1..f - 1, rounds R in 1..16.  A cell is read as its unsigned byte u.
 * Cells with u > 31 take no part: they are not counted in P and are copied unchanged, so the rule is total on any
 * 16 bytes.  One round on a board:
 *   P = the set of the values 1..31 present on the board;  m = max P, 0 for an empty P
 *   if m < f: the board is done
 *   j = the largest value with l <= j < m that is not in P; if there is none: the board is done
 *   every cell with j < u <= 31 becomes u - 1
 * Rounds repeat until the board is done, and at most R times.  shift[i] = the number of rounds applied to board i.
 * What follows, per round applied and so for the whole map:
 *   m falls by exactly one: j < m, so the cells holding m are decremented, and nothing above m exists in P.
 *   For any two cells, <, == and > between their values are the same before and after: j was absent, so
 *   j + 1 -> j collides with nothing, and u -> u - [u > j] is strictly increasing on the values present (cells
 *   with u > 31 stay above every cell that takes part).
 *   Empty cells stay empty (j >= l >= 1), and cells with a value <= j are untouched.
 *   Hence the legal-move mask of the translated board is that of the original, move(., a) moves the same tiles
 *   to the same cells (move(D(b), a) = D(move(b, a)) cell for cell, D the map u -> u - [j < u <= 31] of the
 *   round), and a best chosen on the translated board is a legal action of the original.
 *   shift == 0 leaves the board byte for byte.
 *   f = 15, l = 1, R = 1 is the rule of the paper (once a 32768 is on the board): 32768, 16384, 8192, 2048 becomes
 *   16384, 8192, 4096, 2048.
 * What is NOT preserved: the merge points of halved tiles are halved; deeper in a search a merge into the value j
 * can meet the former j + 1, which the original board would not merge.  So the q of a translated board are values
 * of that board: useful for ranking the moves, not scores of the original.
 */
#ifndef G2048_NTUPLE_H
#define G2048_NTUPLE_H

#include "g2048.h"

#ifdef __cplusplus
extern "C" {
#endif

#define G2048_NT_MAX_TUPLES 8
#define G2048_NT_MAX_LEN 6
#define G2048_NT_FRAC_BITS 12 /* S = 4096: values are points x S */
#define G2048_NT_MAX_TRACE 4        /* the longest eligibility trace of the lambda step */
#define G2048_NT_MAX_LAMBDA_SHIFT 7 /* lambda = 2^-lambda_shift, lambda_shift in 1..7 */
#define G2048_NT_MAX_STAGES 16      /* G, the number of stages of a net, is in 1..16 */

typedef struct g2048_ntuple_net { /* host struct, read during the call */
    int32_t num_tuples;           /* T in 1..8 */
    int32_t tuple_len;            /* K in 1..6, the same for every tuple */
    int32_t cells[48];            /* cells[K t + j] = 4 row + col, 0..15; cells within a tuple distinct */
    int32_t *weights;             /* device int32 [T][16^K], 16-B aligned */
} g2048_ntuple_net;

typedef struct g2048_ntuple_staged_net { /* host struct, read during the call: a net with stages (Stages, above) */
    g2048_ntuple_net net; /* as above, but weights is device int32 [G][T][16^K] */
    uint64_t stage_map;   /* nibble m (bits 4 m ..) = the stage of a board whose largest clamped exponent is m; 0: one stage */
} g2048_ntuple_staged_net;

/* T x 16^K, the number of int32 weights; 0 for a net the calls below would refuse (a null net, T, K or
   a cell out of range, a repeated cell in a tuple, null or misaligned weights). */
size_t g2048_ntuple_weight_count(const g2048_ntuple_net *net);

/* value[i] = V(boards[i]), int64 [n].  boards [n,16] is only read.  0 <= n < 2^31.
   G2048_EINVAL for a net g2048_ntuple_weight_count refuses, n out of range, null or misaligned
   boards, a null value. */
int g2048_ntuple_value(g2048_stream_t stream, const g2048_ntuple_net *net, const int8_t *boards, int64_t *value,
                       int64_t n);

/* The choice on n boards: q int64 [n][4] (16-B aligned), legal / best uint8 [n]; each of the three is
   nullable, but not all three at once.  boards [n,16] is only read.  0 <= n < 2^31.  G2048_EINVAL as
   g2048_ntuple_value, for a misaligned q and for three null outputs. */
int g2048_ntuple_choose(g2048_stream_t stream, const g2048_ntuple_net *net, const int8_t *boards, int64_t *q,
                        uint8_t *legal, uint8_t *best, int64_t n);

/* `steps` TD steps of n envs learning in parallel on one net, two launches per step (evaluate, then
   update and step; stream order between them is the read-before-write rule).  boards / after [n,16]
   int8 (16-B aligned), pending uint8 [n], run_score int64 [n] are read at the start and carried:
   a second call continues the first when the counter is advanced by `steps`.  stats (nullable) int64
   [4] = {games finished, sum of their scores, largest finished score, updates applied}: accumulated,
   not zeroed (the largest by maximum).  workspace: g2048_ntuple_td_workspace_bytes(n) bytes, 16-B
   aligned, contents ignored and overwritten (0 is returned for an n the call would refuse).
   G2048_EINVAL for a net g2048_ntuple_weight_count refuses, steps < 1, lr_shift outside 1..30, n < 0 or
   n >= 2^28, an rng mode other than Philox (or a misaligned counter_dev), null or misaligned boards /
   after, a null pending / run_score, a null, misaligned or too small workspace. */
size_t g2048_ntuple_td_workspace_bytes(int64_t n);
int g2048_ntuple_td(g2048_stream_t stream, const g2048_ntuple_net *net, int8_t *boards, int8_t *after,
                    uint8_t *pending, int64_t *run_score, int64_t n, int64_t steps, int32_t lr_shift,
                    const g2048_rng *rng, int64_t *stats, void *workspace, size_t workspace_bytes);

/* `steps` TC steps (the TC step, above) of n envs on one net and its accumulators tc, int64 [T][16^K][2]
   (device, 16-B aligned, read and updated; zero-filled at the start of a run), three launches per step:
   evaluate (reads W), add to W (reads E and A), add to E and A and step the envs; stream order between
   them is the read-before-write rule.  Everything else -- the carried state, stats, the workspace (of
   g2048_ntuple_tc_workspace_bytes(n) bytes), the refusals -- is g2048_ntuple_td's; in addition
   G2048_EINVAL for a null or misaligned tc. */
size_t g2048_ntuple_tc_workspace_bytes(int64_t n);
int g2048_ntuple_tc(g2048_stream_t stream, const g2048_ntuple_net *net, int64_t *tc, int8_t *boards,
                    int8_t *after, uint8_t *pending, int64_t *run_score, int64_t n, int64_t steps,
                    int32_t lr_shift, const g2048_rng *rng, int64_t *stats, void *workspace,
                    size_t workspace_bytes);

/* `steps` lambda steps (the lambda step, above) of n envs on one net.  tc == NULL: rule TD, two launches
   per step (evaluate; add, move the history on and step the envs).  A non-null tc: rule TC on the
   accumulators tc, whose layout and meaning are g2048_ntuple_tc's, three launches per step (evaluate;
   add to W; add to E and A, move the history on and step the envs).  hist int8 [trace_len][n][16]
   (16-B aligned) and hist_len uint8 [n] are carried like after / pending; with trace_len == 0 both may
   be null and the call is g2048_ntuple_td / _tc bit for bit.  Everything else -- the carried state,
   stats, the workspace (of g2048_ntuple_lambda_workspace_bytes(n) bytes), the refusals -- is
   g2048_ntuple_td's; in addition G2048_EINVAL for trace_len outside 0..G2048_NT_MAX_TRACE, lambda_shift
   outside 1..G2048_NT_MAX_LAMBDA_SHIFT, a misaligned tc and, with trace_len > 0, a null or misaligned
   hist or a null hist_len. */
size_t g2048_ntuple_lambda_workspace_bytes(int64_t n);
int g2048_ntuple_lambda(g2048_stream_t stream, const g2048_ntuple_net *net, int64_t *tc, int8_t *boards,
                        int8_t *after, int8_t *hist, uint8_t *hist_len, uint8_t *pending, int64_t *run_score,
                        int64_t n, int64_t steps, int32_t lr_shift, int32_t trace_len, int32_t lambda_shift,
                        const g2048_rng *rng, int64_t *stats, void *workspace, size_t workspace_bytes);

/* Expectimax search of depth 1..3 with V at the leaves (the search, above) on n boards: q int64 [n][4]
   (16-B aligned, required), leaves int64 [n][4] (nullable, 16-B aligned), legal / best uint8 [n]
   (nullable).  boards [n,16] is only read.  form: G2048_EMAX_AUTO / _NARROW (one workgroup per board) /
   _WIDE (one per (board, action, first spawn), depth >= 2) of g2048.h; the results do not depend on
   it, and AUTO picks a form the call accepts.  workspace: g2048_ntuple_search_workspace_bytes(n, depth,
   form) bytes, 16-B aligned, zero-filled by the call itself (0 is returned for arguments the call
   would refuse).  G2048_EINVAL, with nothing enqueued, for a net g2048_ntuple_weight_count refuses,
   depth outside 1..3, an unknown form, WIDE with depth < 2, n < 0 or a lane count (128 n NARROW,
   16384 n WIDE) >= 2^31, a null or misaligned boards / q / workspace, a misaligned leaves, a too small
   workspace. */
size_t g2048_ntuple_search_workspace_bytes(int64_t n, int64_t depth, int32_t form);
int g2048_ntuple_search(g2048_stream_t stream, const g2048_ntuple_net *net, const int8_t *boards, int64_t n,
                        int64_t depth, int32_t form, int64_t *q, int64_t *leaves, uint8_t *legal, uint8_t *best,
                        void *workspace, size_t workspace_bytes);

/* ---- nets with stages (Stages, above).  G x T x 16^K, the number of int32 weights of a staged net; 0 for a
   net the calls below would refuse: what g2048_ntuple_weight_count refuses, and an invalid stage_map. */
size_t g2048_ntuple_staged_weight_count(const g2048_ntuple_staged_net *net);

/* stage[i] = stage(boards[i]), uint8 [n]: 0 for every board when stage_map == 0.  boards [n,16] is only
   read.  0 <= n < 2^31.  G2048_EINVAL for a net g2048_ntuple_staged_weight_count refuses, n out of range,
   null or misaligned boards, a null stage. */
int g2048_ntuple_stage(g2048_stream_t stream, const g2048_ntuple_staged_net *net, const int8_t *boards,
                       uint8_t *stage, int64_t n);

/* Promotion (Stages, above): W[to][j] += W[from][j] for every j < T 16^K, one launch.  G2048_EINVAL for a
   net g2048_ntuple_staged_weight_count refuses, from or to outside 0..G-1, from == to. */
int g2048_ntuple_promote(g2048_stream_t stream, const g2048_ntuple_staged_net *net, int32_t from, int32_t to);

/* The twins of the calls above on a staged net: each is its one-stage call with weights [G][T][16^K] (and
   tc [G][T][16^K][2]) and every after-state evaluated and updated in the tables of its own stage; it
   refuses what that call refuses and a net g2048_ntuple_staged_weight_count refuses.  The workspaces are
   those of the one-stage calls (g2048_ntuple_td_workspace_bytes and the others). */
int g2048_ntuple_staged_value(g2048_stream_t stream, const g2048_ntuple_staged_net *net, const int8_t *boards,
                              int64_t *value, int64_t n);
int g2048_ntuple_staged_choose(g2048_stream_t stream, const g2048_ntuple_staged_net *net, const int8_t *boards,
                               int64_t *q, uint8_t *legal, uint8_t *best, int64_t n);
int g2048_ntuple_staged_td(g2048_stream_t stream, const g2048_ntuple_staged_net *net, int8_t *boards, int8_t *after,
                           uint8_t *pending, int64_t *run_score, int64_t n, int64_t steps, int32_t lr_shift,
                           const g2048_rng *rng, int64_t *stats, void *workspace, size_t workspace_bytes);
int g2048_ntuple_staged_tc(g2048_stream_t stream, const g2048_ntuple_staged_net *net, int64_t *tc, int8_t *boards,
                           int8_t *after, uint8_t *pending, int64_t *run_score, int64_t n, int64_t steps,
                           int32_t lr_shift, const g2048_rng *rng, int64_t *stats, void *workspace,
                           size_t workspace_bytes);
int g2048_ntuple_staged_lambda(g2048_stream_t stream, const g2048_ntuple_staged_net *net, int64_t *tc, int8_t *boards,
                               int8_t *after, int8_t *hist, uint8_t *hist_len, uint8_t *pending, int64_t *run_score,
                               int64_t n, int64_t steps, int32_t lr_shift, int32_t trace_len, int32_t lambda_shift,
                               const g2048_rng *rng, int64_t *stats, void *workspace, size_t workspace_bytes);
int g2048_ntuple_staged_search(g2048_stream_t stream, const g2048_ntuple_staged_net *net, const int8_t *boards,
                               int64_t n, int64_t depth, int32_t form, int64_t *q, int64_t *leaves, uint8_t *legal,
                               uint8_t *best, void *workspace, size_t workspace_bytes);

/* ---- the carousel (Carousel, above): the arrays carried beside those of the lambda step */
typedef struct g2048_ntuple_carousel { /* host struct, read during the call; all device pointers */
    int8_t *pool;    /* [G][n][16], 16-B aligned */
    uint8_t *valid;  /* [n][16],    16-B aligned */
    uint8_t *next;   /* [n] */
    uint8_t *origin; /* [n] */
} g2048_ntuple_carousel;

/* `steps` carousel steps of n envs on a staged net: g2048_ntuple_staged_lambda's arguments in its order, its
   refusals and its launches per step (two under rule TD, three under TC), and car.  stats (nullable) int64 [8]
   = {full games finished, sum of their scores, largest of them, updates applied, restarted games finished,
   sum of their points since the restart, snapshots recorded, restarts}: accumulated, not zeroed.  workspace:
   g2048_ntuple_carousel_workspace_bytes(n) bytes (0 for an n the call would refuse).  In addition
   G2048_EINVAL, with n > 0, for a null car, a null member of it, a misaligned pool or valid and a workspace
   smaller than that. */
size_t g2048_ntuple_carousel_workspace_bytes(int64_t n);
int g2048_ntuple_staged_carousel(g2048_stream_t stream, const g2048_ntuple_staged_net *net, int64_t *tc, int8_t *boards,
                                 int8_t *after, int8_t *hist, uint8_t *hist_len, uint8_t *pending, int64_t *run_score,
                                 int64_t n, int64_t steps, int32_t lr_shift, int32_t trace_len, int32_t lambda_shift,
                                 const g2048_rng *rng, const g2048_ntuple_carousel *car, int64_t *stats, void *workspace,
                                 size_t workspace_bytes);

/* ---- optimistic initialisation (Optimistic initialisation, above).  fill: W[j] = w0 for every weight of the net,
   j < T 16^K (staged: j < G T 16^K), one launch; any int32 w0; nothing outside the tables is written.
   G2048_EINVAL for a net g2048_ntuple_weight_count (staged: g2048_ntuple_staged_weight_count) refuses. */
int g2048_ntuple_fill(g2048_stream_t stream, const g2048_ntuple_net *net, int32_t w0);
int g2048_ntuple_staged_fill(g2048_stream_t stream, const g2048_ntuple_staged_net *net, int32_t w0);

/* Promotion over a start: W[to][j] += W[from][j] - base for every j < T 16^K, one launch; any int32 base, base 0
   is g2048_ntuple_promote.  The refusals are g2048_ntuple_promote's. */
int g2048_ntuple_promote_from(g2048_stream_t stream, const g2048_ntuple_staged_net *net, int32_t from, int32_t to,
                              int32_t base);

/* ---- tile-downgrading (Tile-downgrading, above): out[i] = boards[i] after at most `rounds` rounds with from_exp
   and lo_exp, shift[i] (nullable, uint8 [n]) = the rounds applied.  boards / out int8 [n,16], 16-B aligned;
   out == boards is allowed (in place: every board is read and written by its own lane only), any other overlap is
   not.  One launch, no workspace.  0 <= n < 2^31.  G2048_EINVAL for from_exp outside 2..31, lo_exp outside
   1..from_exp - 1, rounds outside 1..16, n out of range, null or misaligned boards or out. */
int g2048_ntuple_downgrade(g2048_stream_t stream, const int8_t *boards, int8_t *out, uint8_t *shift, int64_t n,
                           int32_t from_exp, int32_t lo_exp, int32_t rounds);

#ifdef __cplusplus
}
#endif
#endif /* G2048_NTUPLE_H */
