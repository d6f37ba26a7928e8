"""Numpy restatement of the stage between two of `imagine`'s one-step rollouts (csrc/imagine.hip: imagine_select_kernel,
cadm_imagine_select) -- test infrastructure shared by tests/test_imagine_ref.py (CPU) and tests/test_gpu_imagine.py.

Everything here is exact: the draw is integer arithmetic on oracle/philox.py's words, the selection and the broadcast are copies, the
health test is two float32 comparisons per constraint, the state machine is boolean, and the disagreement is
tests/uncertainty_ref.py's float32 walk of the variance chain (kind "epistemic", form "var", no cap) on the step's particles.  So the
kernel is held to it bit for bit (include/cadm_hip.h, "Imagined rollouts")."""
import numpy as np

import uncertainty_ref as uref
from oracle import philox

F = np.float32
STREAM_IMAGINE = 6          # csrc/common.h CADM_STREAM_IMAGINE: the particle draw
STREAM_IMAGINE_ACT = 7      # csrc/common.h CADM_STREAM_IMAGINE_ACT: the action noise
IMAGINE_IT = 0xF00000       # csrc/planner.h CADM_IMAGINE_IT


def words(seed, call, rows, t):
    """word 0 of Philox4x32-10 keyed (seed, call), counter (row, t, 0, STREAM_IMAGINE), for the row ids `rows` -> uint32 of their shape"""
    rows = np.asarray(rows, dtype=np.uint32)
    r = philox.philox4x32_10(philox._ctr(rows, np.uint32(t), np.uint32(0), np.uint32(STREAM_IMAGINE)), philox._key(seed, call, rows.shape))
    return r[..., 0]


def select(w0, p):
    """sel = (uint64(w0) * p) >> 32: 0 .. p - 1"""
    return ((np.asarray(w0, dtype=np.uint32).astype(np.uint64) * np.uint64(p)) >> np.uint64(32)).astype(np.int32)


def draws(seed, call, m, n, k, p):
    """sel [k, m, n] of a whole call: row = mi * n + j"""
    rows = np.arange(m * n, dtype=np.uint32).reshape(m, n)
    return np.stack([select(words(seed, call, rows, t), p) for t in range(k)])


def xi(seed, call, rows, t, A):
    """the action noise [rows, A] float32 of step t: tests/policy_ref.py's `xi` with every row drawn and the stream word of imagine"""
    row = np.arange(rows, dtype=np.uint32)
    ng = (A + 3) // 4
    out = np.empty((rows, 4 * ng), F)
    for g in range(ng):
        r = philox.philox4x32_10(philox._ctr(row, np.uint32(t), np.uint32(g), np.uint32(STREAM_IMAGINE_ACT)), philox._key(seed, call, row.shape))
        out[..., 4 * g], out[..., 4 * g + 1] = philox.box_muller(philox.u01(r[..., 0]), philox.u01(r[..., 1]))
        out[..., 4 * g + 2], out[..., 4 * g + 3] = philox.box_muller(philox.u01(r[..., 2]), philox.u01(r[..., 3]))
    return out[..., :A]


def disagreement(nxt, E, w=None):
    """u [R] float32 of the particles nxt [R, p, D]: uncertainty_ref.emulate32's step cost of a one-step trajectory, a non-finite
    result stored as +inf"""
    nxt = np.asarray(nxt, F)
    u, _ = uref.emulate32(nxt[None, :, None], E, "epistemic", w=w, form="var")
    u = u[:, 0, 0]
    return np.where(np.isfinite(u), u, F(np.inf)).astype(F)


def healthy(x, constraints):
    """[R] bool: x[dim] > lo and x[dim] < hi in float32 for every constraint dict(dim=, lo=, hi=); a value on a bound violates, NaN too"""
    x = np.asarray(x, F)
    ok = np.ones(x.shape[:-1], bool)
    for c in constraints or ():
        v = x[..., int(c["dim"])]
        with np.errstate(invalid="ignore"):
            ok &= (v > F(c.get("lo", -np.inf))) & (v < F(c.get("hi", np.inf)))
    return ok


def select_step(nxt, rows1, state, alive, sel, E, constraints=None, w=None, length=None):
    """One step of the stage on R rows: nxt [R, p, D], rows1 [R, p], state [R, D] (states[t]), alive [R], sel [R] -> dict(state, rew, done,
    valid, member, disagreement, alive, length, bcast) as `HipEngine.imagine_select` returns them."""
    nxt, rows1, state = np.asarray(nxt, F), np.asarray(rows1, F), np.asarray(state, F)
    R, p, D = nxt.shape
    sel = np.asarray(sel, np.int64)
    was = np.asarray(alive).astype(bool)
    s1 = nxt[np.arange(R), sel]                                  # [R, D]
    finite = np.isfinite(s1).all(axis=1)
    ok = healthy(s1, constraints)
    u = disagreement(nxt, E, w)
    valid = was & finite
    done = valid & ~ok
    new = np.where(valid[:, None], s1, state).astype(F)
    length = np.zeros((R,), np.int32) if length is None else np.asarray(length, np.int32)
    return dict(state=new, rew=np.where(valid, rows1[np.arange(R), sel], F(0)).astype(F), done=done.astype(np.uint8),
                valid=valid.astype(np.uint8), member=np.where(was, sel // (p // E), -1).astype(np.int32),
                disagreement=np.where(was, u, F(0)).astype(F), alive=(valid & ~done).astype(np.uint8),
                length=(length + valid).astype(np.int32), bcast=np.repeat(new[:, None, :], p, axis=1))


def run_steps(state0, nexts, rows1s, sels, E, constraints=None, w=None):
    """The state machine over k steps on given particles: state0 [R, D], nexts [k, R, p, D], rows1s [k, R, p], sels [k, R] -> dict of
    stacked outputs (states [k + 1, R, D]; rew, done, valid, member, disagreement [k, R]; length, alive [R]).  What a rollout would have
    made of a dead row's frozen state is whatever `nexts` holds there: it is ignored."""
    k = len(nexts)
    states, alive, length = [np.asarray(state0, F)], np.ones((len(state0),), np.uint8), None
    cols = {name: [] for name in ("rew", "done", "valid", "member", "disagreement")}
    for t in range(k):
        o = select_step(nexts[t], rows1s[t], states[-1], alive, sels[t], E, constraints, w, length)
        states.append(o["state"])
        alive, length = o["alive"], o["length"]
        for name in cols:
            cols[name].append(o[name])
    out = {name: np.stack(v) for name, v in cols.items()}
    out.update(states=np.stack(states), length=length, alive=alive)
    return out


# ---------------------------------------------------------------------------------------------------------------------- the stage's groups
GROUP, LDS_BUDGET = 16, 48 * 1024      # csrc/imagine.hip IMG_GROUP, IMG_LDS_BUDGET


def lds_bytes(G, p, D):
    """csrc/imagine.hip img_lds_bytes: the tile of G p D floats, G D variances and D weights, each padded to 4 floats, and G ints"""
    pad4 = lambda v: (v + 3) & ~3
    return 4 * (pad4(G * p * D) + pad4(G * D) + pad4(D) + G)


def group(p, D):
    """csrc/imagine.hip img_group: the rows a workgroup of the select stage owns -- 16, fewer where the tile would not fit 48 KiB
    (0: not even one row's, and the stage is refused)"""
    return max(G for G in range(0, GROUP + 1) if G == 0 or lds_bytes(G, p, D) <= LDS_BUDGET)


# The kernel-level engines of tests/test_gpu_imagine_envelope.py -- name: (env, D, p, the group, the groups of its 37 rows) -- at which the
# budget cuts the group below 16; "wide255": one row's tile of 12337 floats is beyond the 12288 of the budget
STAGE_ENGINES = {
    "slim35": ("slim_humanoid", 45, 35, 7, [7] * 5 + [2]),      # p D = 1575, odd: group starts of every alignment in one launch
    "hc50": ("halfcheetah", 18, 50, 13, [13, 13, 11]),          # p D = 900
    "wide30": ("widest", 48, 30, 8, [8] * 4 + [5]),             # p D = 1440
    "wide125": ("widest", 48, 125, 2, [2] * 18 + [1]),          # p D = 6000; PE = 25; p > S = 256 / 48: the broadcast walk's carry
    "wide255": ("widest", 48, 255, 0, None),
}
# where the stage test embeds its 37 rows in a batch of 150 so that their place inside a group moves: row 100, which is no multiple of 7, 13
# or 8 -- and row 101 where the group is 2
STAGE_AT = {"wide125": 101}
