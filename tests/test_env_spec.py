"""CPU: user-declared envs (cadm_amd/env_spec.py EnvDecl) -- the numpy closures against the oracle's built-in closures, validation,
the generated header and its hash, a cross-compiled spec rollout module, and the library's envelope check of a spec-kind config."""
import ctypes
import os
import re

import numpy as np
import pytest

from cadm_amd import _lib
from cadm_amd.env_spec import TERMS, WHEN, EnvDecl, restate
from cadm_amd.envs import resolve_env_kind, make_env_spec
from helpers import CORNER_DECLS, corner_spec
from oracle.envs import make_env

KINDS = ("halfcheetah", "ant", "slim_humanoid")


def hopper_like():
    return EnvDecl(11, 3, preproc=["drop", "sincos", "id", "id", "sincos", "id", "id", "id", "id", "id", "id"],
                   postproc=["add"] * 5 + ["replace"] + ["add"] * 5,
                   reward=[dict(kind="linear", dim=5), dict(kind="square", dim=3, w=-0.5, when="next_obs"),
                           dict(kind="abs", dim=10, w=-0.1), dict(kind="inside", dim=0, w=1.0, lo=-0.5, hi=0.5, when="next_obs"),
                           dict(kind="outside", dim=2, w=-1.0, lo=-0.2, hi=0.2), dict(kind="linear", dim=4, w=0.3, when="next_obs")],
                   ctrl_cost=0.001, bonus=1.0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restated_closures_equal_the_oracle(kind, dtype):
    spec, ref = restate(kind), make_env(kind)
    assert (spec.obs_dim, spec.act_dim, spec.proc_obs_dim) == (ref.obs_dim, ref.act_dim, ref.proc_obs_dim)
    rng = np.random.default_rng(3)
    D, A = ref.obs_dim, ref.act_dim
    obs = (2.0 * rng.standard_normal((5, 7, D))).astype(dtype)
    nxt = (2.0 * rng.standard_normal((5, 7, D))).astype(dtype)
    pred = rng.standard_normal((5, 7, D)).astype(dtype)
    act = rng.uniform(-1, 1, (5, 7, A)).astype(dtype)
    obs[..., 1] = rng.uniform(0.5, 2.5, (5, 7)).astype(dtype)      # both sides of slim humanoid's alive window
    for mine, theirs in ((spec.obs_preproc(obs), ref.obs_preproc(obs)), (spec.obs_postproc(obs, pred), ref.obs_postproc(obs, pred)),
                         (spec.targ_proc(obs, nxt), ref.targ_proc(obs, nxt))):
        assert mine.dtype == theirs.dtype and mine.shape == theirs.shape
        assert np.array_equal(mine.view(np.uint8), theirs.view(np.uint8))
    r, rr = spec.reward(obs, act, nxt), ref.reward(obs, act, nxt)
    assert r.dtype == rr.dtype
    ulp = np.spacing(np.abs(rr).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(r.astype(np.float64) - rr.astype(np.float64)) <= ulp)


def test_new_env_closures():
    spec = hopper_like()
    assert spec.proc_obs_dim == 12
    rng = np.random.default_rng(0)
    obs, nxt, act = rng.standard_normal((4, 11)), rng.standard_normal((4, 11)), rng.uniform(-1, 1, (4, 3))
    pre = spec.obs_preproc(obs)
    assert np.array_equal(pre[:, :3], np.stack([np.sin(obs[:, 1]), np.cos(obs[:, 1]), obs[:, 2]], -1))
    assert np.array_equal(pre[:, 4:6], np.stack([np.sin(obs[:, 4]), np.cos(obs[:, 4])], -1))
    delta = spec.targ_proc(obs, nxt)
    assert delta[:, 5].tolist() == nxt[:, 5].tolist()
    assert np.array_equal(spec.obs_postproc(obs, delta)[:, 5], nxt[:, 5])
    want = (obs[:, 5] - 0.001 * np.sum(act ** 2, -1) + 1.0 - 0.5 * nxt[:, 3] ** 2 - 0.1 * np.abs(obs[:, 10])
            + ((nxt[:, 0] > -0.5) & (nxt[:, 0] < 0.5)) - ((obs[:, 2] > 0.2).astype(float) + (obs[:, 2] < -0.2)) + 0.3 * nxt[:, 4])
    np.testing.assert_allclose(spec.reward(obs, act, nxt), want, rtol=1e-12, atol=1e-12)


def test_validation():
    with pytest.raises(ValueError, match="reads obs dim 11"):
        EnvDecl(11, 3, reward=[dict(kind="linear", dim=11)])
    with pytest.raises(ValueError, match="at most 2 features"):
        EnvDecl(3, 1, preproc=["id", ("id", "sin", "cos"), "id"])
    with pytest.raises(ValueError, match="one entry per obs dim"):
        EnvDecl(3, 1, preproc=["id", "id"])
    with pytest.raises(ValueError, match="expected one of"):
        EnvDecl(3, 1, preproc=["id", "tan", "id"])
    with pytest.raises(ValueError, match="lo < hi"):
        EnvDecl(3, 1, reward=[dict(kind="inside", dim=0, lo=1.0, hi=1.0)])
    with pytest.raises(ValueError, match="kind 'cube'"):
        EnvDecl(3, 1, reward=[dict(kind="cube", dim=0)])
    with pytest.raises(ValueError, match="when 'later'"):
        EnvDecl(3, 1, reward=[dict(kind="abs", dim=0, when="later")])
    with pytest.raises(ValueError, match=r"D <= 48"):
        EnvDecl(49, 3)
    with pytest.raises(ValueError, match=r"A <= 24"):
        EnvDecl(10, 25)
    with pytest.raises(ValueError, match=r"P <= 64"):
        EnvDecl(40, 3, preproc="sincos")
    with pytest.raises(ValueError, match="P=0"):
        EnvDecl(2, 1, preproc="drop")
    EnvDecl(45, 17, preproc="id")                     # slim humanoid's shape is inside the envelope
    EnvDecl(48, 24, preproc=["sincos"] * 16 + ["id"] * 32)


def test_resolution_of_specs():
    spec = hopper_like()
    assert resolve_env_kind(spec) is spec

    class UserEnv:                                    # a simulator that declares its closures
        cadm_env_spec = spec

    class Wrapper:
        def __init__(self, e):
            self.wrapped_env = e
    assert resolve_env_kind(Wrapper(Wrapper(UserEnv()))) is spec
    assert resolve_env_kind(make_env_spec("ant")) == "ant"

    class DuckOnly:                                   # right duck type, no spec, no compiled-in class: still refused
        observation_space = spec.observation_space
        action_space = spec.action_space
        proc_observation_space_dims = spec.proc_obs_dim
        obs_preproc, obs_postproc, targ_proc, reward = spec.obs_preproc, spec.obs_postproc, spec.targ_proc, spec.reward
    with pytest.raises(ValueError, match="compiled-in env kind"):
        resolve_env_kind(Wrapper(DuckOnly()))


def test_header_and_hash():
    a, b = hopper_like(), hopper_like()
    assert a.header() == b.header() and a.hash == b.hash and a == b
    h = a.header()
    assert "#define CADM_SPEC_D 11" in h and "#define CADM_SPEC_P 12" in h and "#define CADM_SPEC_NTERMS 6" in h
    assert "asm" not in h and "__" not in h                   # data tables only
    base = dict(obs_dim=11, act_dim=3, preproc=list(a.preproc), postproc=list(a.postproc),
                reward=[dict(kind=k, dim=d, when=w, w=wt, **({"lo": lo, "hi": hi} if k in ("inside", "outside") else {}))
                        for (k, d, w, wt, lo, hi) in a.terms], ctrl_cost=a.ctrl_cost, bonus=a.bonus)
    assert EnvDecl(**base).hash == a.hash

    def variant(**kw):
        v = {k: (list(x) if isinstance(x, list) else x) for k, x in base.items()}
        v["reward"] = [dict(t) for t in base["reward"]]
        v.update(kw)
        return v
    variants = [variant(act_dim=4), variant(ctrl_cost=0.002), variant(bonus=0.5),
                variant(preproc=["drop", "sincos", "id", "drop", "sincos"] + ["id"] * 6),
                variant(postproc=["add"] * 11)]
    for field, value in (("w", 2.0), ("dim", 6), ("when", "next_obs"), ("kind", "abs")):
        v = variant()
        v["reward"][0][field] = value
        variants.append(v)
    v = variant()
    v["reward"][3]["hi"] = 0.6
    variants.append(v)
    v = variant()
    v["reward"] = v["reward"][::-1]
    variants.append(v)
    hashes = {EnvDecl(**v).hash for v in variants}
    assert a.hash not in hashes and len(hashes) == len(variants)
    for v in variants:
        assert EnvDecl(**v).header() != h
    lo, hi = a.hash_words
    assert (lo & 0xFFFFFFFF) | ((hi & 0xFFFFFFFF) << 32) == a.hash64


def test_env_spec_of_a_restated_kind_is_its_restated_spec():
    """envs.EnvSpec of halfcheetah / ant / slim humanoid: dims and numpy closures of restate(kind) (bit for bit, float32 and float64),
    but it resolves to its NAME (the kernels compiled into the library, no JIT build).  Cartpole and pendulum: identity closures."""
    rng = np.random.default_rng(4)
    for kind in KINDS + ("cripple_halfcheetah",):
        env, spec = make_env_spec(kind), restate(kind)
        assert not hasattr(env, "cadm_env_spec") and env.cadm_env_kind == env.kind == kind and resolve_env_kind(env) == kind
        assert (env.observation_space.shape, env.action_space.shape, env.proc_observation_space_dims) == ((spec.obs_dim,), (spec.act_dim,), spec.proc_obs_dim)
        ref = make_env(kind)
        for dtype in (np.float32, np.float64):
            obs, pred, nxt = (rng.standard_normal((3, 5, spec.obs_dim)).astype(dtype) for _ in range(3))
            for mine, decl, theirs in ((env.obs_preproc(obs), spec.obs_preproc(obs), ref.obs_preproc(obs)),
                                       (env.obs_postproc(obs, pred), spec.obs_postproc(obs, pred), ref.obs_postproc(obs, pred)),
                                       (env.targ_proc(obs, nxt), spec.targ_proc(obs, nxt), ref.targ_proc(obs, nxt))):
                assert mine.dtype == dtype and mine.shape == theirs.shape
                assert np.array_equal(mine, decl) and np.array_equal(mine.view(np.uint8), theirs.view(np.uint8))
    for kind, dims in (("cartpole", (4, 2, 4)), ("pendulum", (3, 1, 3))):
        env = make_env_spec(kind)
        A = env.action_space.n if kind == "cartpole" else env.action_space.shape[0]
        assert (env.observation_space.shape[0], A, env.proc_observation_space_dims) == dims and resolve_env_kind(env) == kind
        o, q = np.arange(dims[0], dtype=np.float64), np.ones(dims[0])
        assert np.array_equal(env.obs_preproc(o), o) and np.array_equal(env.obs_postproc(o, q), o + q) and np.array_equal(env.targ_proc(o, q), q - o)


def test_jit_cross_compiles_a_spec_module(tmp_path, monkeypatch):
    import json
    from cadm_amd import isa_check, jit
    if not jit.hipcc() or not isa_check.find_objdump():
        pytest.skip("hipcc / llvm-objdump not available")
    monkeypatch.setenv("CADM_JIT_CACHE", str(tmp_path))
    monkeypatch.setattr(jit, "_memo", {})
    spec = hopper_like()
    path = jit.build(_lib.ENV_SPEC, 10, 200, 4, _lib.ACT_KINDS["swish"], _lib.NOISE_INJECT, spec=spec)
    assert spec.hash[:16] in os.path.basename(path) and os.path.exists(path)
    assert open(os.path.join(tmp_path, "spec_" + spec.hash[:16], "cadm_spec_tables.h")).read() == spec.header()
    rep = json.load(open(path + ".isa.json"))
    assert rep["checked"] and rep["problems"] == 0 and rep["kernels"] >= 3, rep
    with pytest.raises(_lib.CadmError, match="needs its env spec"):
        jit.build(_lib.ENV_SPEC, 10, 200, 4, 0, 1)
    # the module reports the spec it was built for
    mod = ctypes.CDLL(path)
    desc = (ctypes.c_int * 10)()
    mod.cadm_jit_describe(desc)
    assert desc[1] == _lib.ENV_SPEC and tuple(desc[8:10]) == spec.hash_words


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _spec_cfg(D, A, P):
    cfg = _lib.Config()
    cfg.abi_version = _lib.ABI_VERSION
    cfg.env_kind = _lib.ENV_SPEC
    cfg.obs_dim, cfg.act_dim, cfg.proc_obs_dim = D, A, P
    cfg.ensemble_size = cfg.n_particles = 1
    cfg.n_hidden, cfg.hidden, cfg.horizon = 4, 200, 30
    return cfg


@pytest.mark.parametrize("dims,bound", [((49, 3, 20), "D=49"), ((0, 3, 20), "D=0"), ((11, 25, 12), "A=25"), ((11, 0, 12), "A=0"),
                                        ((40, 3, 65), "P=65"), ((11, 3, 23), "P=23"), ((11, 3, 0), "P=0")])
def test_ctx_create_refuses_a_spec_outside_the_envelope(lib, dims, bound):
    ctx = ctypes.c_void_p()
    rc = lib.cadm_ctx_create(ctypes.byref(_spec_cfg(*dims)), ctypes.byref(ctx))
    msg = lib.cadm_last_error()
    assert rc == -1 and not ctx.value
    assert b"envelope" in msg and bound.encode() in msg, msg
    cfg = _spec_cfg(11, 3, 12)
    cfg.discrete = 1
    assert lib.cadm_ctx_create(ctypes.byref(cfg), ctypes.byref(ctx)) == -1 and b"continuous" in lib.cadm_last_error()
    cfg = _spec_cfg(11, 3, 12)
    cfg.env_kind = 6
    assert lib.cadm_ctx_create(ctypes.byref(cfg), ctypes.byref(ctx)) == -1 and b"unknown env kind" in lib.cadm_last_error()


def test_spec_struct_layout_matches_header():
    # 3 + 48 + 48 + 1 + 3 * 32 int32, 3 * 32 + 2 float, 2 uint32
    assert ctypes.sizeof(_lib.EnvSpecC) == (3 + 48 + 48 + 1 + 96 + 96 + 2 + 2) * 4
    assert ctypes.sizeof(_lib.Config) == 37 * 4


# ------------------------------------------------------------------------------------------------------------------------------
# the corners of the envelope (tests/helpers.py CORNER_DECLS; run on the GPU by tests/test_gpu_env_spec_envelope.py)
# ------------------------------------------------------------------------------------------------------------------------------
def _restated(decl):
    """The closures of a declaration, restated from its plain lists in float64 (independent of EnvDecl's tables)."""
    D = decl["obs_dim"]
    pre = decl.get("preproc", "id")
    post = decl.get("postproc", "add")
    pre = [pre] * D if isinstance(pre, str) else list(pre)
    post = [post] * D if isinstance(post, str) else list(post)

    def preproc(obs):
        cols = []
        for d in range(D):
            if pre[d] == "id":
                cols.append(obs[..., d])
            elif pre[d] == "sincos":
                cols += [np.sin(obs[..., d]), np.cos(obs[..., d])]
        return np.stack(cols, -1)

    def postproc(obs, pred):
        return np.stack([pred[..., d] if post[d] == "replace" else obs[..., d] + pred[..., d] for d in range(D)], -1)

    def targ(obs, nxt):
        return np.stack([nxt[..., d] if post[d] == "replace" else nxt[..., d] - obs[..., d] for d in range(D)], -1)

    def term(t, obs, nxt):
        x = (nxt if t.get("when", "obs") == "next_obs" else obs)[..., t["dim"]]
        w = t.get("w", 1.0)
        if t["kind"] == "linear":
            return w * x
        if t["kind"] == "square":
            return w * x * x
        if t["kind"] == "abs":
            return w * np.abs(x)
        if t["kind"] == "inside":
            return w * ((x > t["lo"]) & (x < t["hi"]))
        return w * ((x > t["hi"]).astype(float) + (x < t["lo"]))

    def reward(obs, act, nxt):
        r = sum((term(t, obs, nxt) for t in decl["reward"]), np.zeros(obs.shape[:-1]))
        return r - decl.get("ctrl_cost", 0.0) * np.sum(act * act, -1) + decl.get("bonus", 0.0)
    return preproc, postproc, targ, reward


# the first term's pair, and the pre-step terms on it that the kernels sum first (before the ctrl cost and the bonus)
FIRST_PAIR_GROUP = {"widest": [0, 1, 30], "tiny": [], "tiny_sincos": [0], "odd_tail": [0], "first_next": []}


@pytest.mark.parametrize("corner", sorted(CORNER_DECLS))
def test_corner_closures_match_a_float64_restatement(corner):
    decl, spec = CORNER_DECLS[corner], corner_spec(corner)
    D, A = decl["obs_dim"], decl["act_dim"]
    preproc, postproc, targ, reward = _restated(decl)
    rng = np.random.default_rng(5)
    obs, nxt, pred = (1.5 * rng.standard_normal((6, 9, D)) for _ in range(3))
    act = rng.uniform(-1, 1, (6, 9, A))
    assert spec.proc_obs_dim == preproc(obs).shape[-1]
    assert np.array_equal(spec.obs_preproc(obs), preproc(obs))
    assert np.array_equal(spec.obs_postproc(obs, pred), postproc(obs, pred))
    assert np.array_equal(spec.targ_proc(obs, nxt), targ(obs, nxt))
    assert np.array_equal(spec.obs_postproc(obs, spec.targ_proc(obs, nxt)), postproc(obs, targ(obs, nxt)))
    np.testing.assert_allclose(spec.reward(obs, act, nxt), reward(obs, act, nxt), rtol=1e-12, atol=1e-12)
    # float32: the kernels' grouping, term by term -- ((first pair's pre-step terms) - c ctrl) + bonus, then the rest in order
    o32, n32, a32 = obs.astype(np.float32), nxt.astype(np.float32), act.astype(np.float32)
    terms = decl["reward"]
    head = FIRST_PAIR_GROUP[corner]
    assert head == [k for k, t in enumerate(terms) if t["dim"] >> 1 == terms[0]["dim"] >> 1 and t.get("when", "obs") == "obs"]
    f32 = np.float32

    def t32(t):
        x = (n32 if t.get("when", "obs") == "next_obs" else o32)[..., t["dim"]]
        w = f32(t.get("w", 1.0))
        if t["kind"] == "linear":
            return w * x
        if t["kind"] == "square":
            return w * (x * x)
        if t["kind"] == "abs":
            return w * np.abs(x)
        if t["kind"] == "inside":
            return np.where((x > f32(t["lo"])) & (x < f32(t["hi"])), w, f32(0))
        return w * ((x > f32(t["hi"])).astype(f32) + (x < f32(t["lo"])).astype(f32))
    r = np.zeros(o32.shape[:-1], f32)
    for i, k in enumerate(head):
        r = t32(terms[k]) if i == 0 else r + t32(terms[k])
    if decl.get("ctrl_cost", 0.0):
        r = r - f32(decl["ctrl_cost"]) * np.sum(np.square(a32), -1)
    if decl.get("bonus", 0.0):
        r = r + f32(decl["bonus"])
    for k, t in enumerate(terms):
        if k not in head:
            r = r + t32(t)
    got = spec.reward(o32, a32, n32)
    assert got.dtype == np.float32 and np.array_equal(got, r)


def test_widest_header_masks_and_terms():
    decl, spec = CORNER_DECLS["widest"], corner_spec("widest")
    h = spec.header()
    for k, v in (("D", 48), ("A", 24), ("P", 64), ("NTERMS", 32)):
        assert "#define CADM_SPEC_%s %d\n" % (k, v) in h
    masks = {k: int(re.search(r"#define CADM_SPEC_%s_MASK 0x([0-9a-f]{16})ull" % k, h).group(1), 16) for k in ("DROP", "SINCOS", "REPLACE")}
    for name, field, value in (("DROP", "preproc", "drop"), ("SINCOS", "preproc", "sincos"), ("REPLACE", "postproc", "replace")):
        want = {d for d in range(48) if decl[field][d] == value}
        assert {d for d in range(64) if (masks[name] >> d) & 1} == want, name
    assert {d for d in range(32, 48) if (masks["SINCOS"] >> d) & 1} == {32, 34, 37, 39, 42, 43, 45, 46, 47}
    assert {d for d in range(32, 48) if (masks["DROP"] >> d) & 1} == {40}
    assert {d for d in range(32, 48) if (masks["REPLACE"] >> d) & 1} == {33, 40, 47}
    table = re.search(r"#define CADM_SPEC_TERMS (.*)\n", h).group(1)
    got = [tuple(int(x) for x in e.split(",")[:3]) for e in re.findall(r"\{([^}]*)\}", table)]
    assert got == [(TERMS[t["kind"]], t["dim"], WHEN[t.get("when", "obs")]) for t in decl["reward"]]
    c = spec.to_c()
    assert c.n_terms == 32 and list(c.term_dim)[:32] == [t["dim"] for t in decl["reward"]]
    with pytest.raises(ValueError, match="33 reward terms, at most 32"):
        EnvDecl(**dict(decl, reward=decl["reward"] + [dict(kind="linear", dim=0)]))


# the widest spec in both noise modes that draw or read noise, every other corner in one mode (about 17 s of hipcc each)
CORNER_MODULES = [("widest", 10, _lib.NOISE_PHILOX), ("widest", 10, _lib.NOISE_INJECT), ("widest", 0, _lib.NOISE_NONE),
                  ("tiny", 10, _lib.NOISE_INJECT), ("odd_tail", 10, _lib.NOISE_PHILOX), ("first_next", 10, _lib.NOISE_NONE)]


def test_jit_cross_compiles_the_corner_modules(tmp_path, monkeypatch):
    import json
    from concurrent.futures import ThreadPoolExecutor
    from cadm_amd import isa_check, jit
    if not jit.hipcc() or not isa_check.find_objdump():
        pytest.skip("hipcc / llvm-objdump not available")
    monkeypatch.setenv("CADM_JIT_CACHE", str(tmp_path))
    monkeypatch.setattr(jit, "_memo", {})
    jit.cache_dir(), jit._build_key()

    def build(job):
        corner, C, noise = job
        return jit.build(_lib.ENV_SPEC, C, 200, 4, _lib.ACT_KINDS["swish"], noise, spec=corner_spec(corner))
    with ThreadPoolExecutor(max_workers=max(1, min(len(CORNER_MODULES), os.cpu_count() or 1))) as ex:
        paths = list(ex.map(build, CORNER_MODULES))
    for (corner, C, noise), path in zip(CORNER_MODULES, paths):
        spec = corner_spec(corner)
        rep = json.load(open(path + ".isa.json"))
        assert rep["checked"] and rep["problems"] == 0 and rep["kernels"] >= 3, rep
        # scratch use is a performance defect, not asserted: printed so that a change which moves the spills shows up
        print("%s C=%d noise=%d: scratch %s" % (corner, C, noise, rep["scratch"] or "none"))
        mod = ctypes.CDLL(path)
        desc = (ctypes.c_int * 10)()
        mod.cadm_jit_describe(desc)
        assert desc[1] == _lib.ENV_SPEC and tuple(desc[8:10]) == spec.hash_words
