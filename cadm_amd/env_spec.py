"""User-declared envs: the four closures of an env as a small declarative spec.

The reference's model class takes any env object that provides ``obs_preproc``, ``obs_postproc``, ``targ_proc`` and
``tf_reward_fn()`` (cadm/dynamics/mlp_cadm_ensemble_cem_dynamics.py:95-102,185-187).  The HIP kernels cannot
trace a Python closure, so an env that is not one of the compiled-in kinds (envs.CLASS_TO_KIND) describes its closures with an
``EnvDecl``; the library compiles them into a rollout module of its own (cadm_amd/jit.py: the generated ``cadm_spec_tables.h``
feeds csrc/env_tables.h) and uploads the preprocessing table the training kernels read (``cadm_set_env_spec``).

What a spec expresses (continuous actions only):
  * ``preproc``: per obs dim ``"id"``, ``"drop"`` or ``"sincos"`` (sin then cos); the features appear in dim order, P is their count;
  * ``postproc``: per obs dim ``"add"`` (next = obs + delta) or ``"replace"`` (next = delta); ``targ_proc`` follows from it;
  * ``reward``: a list of terms, each reading ONE obs dim of the pre-step (``when="obs"``) or post-step (``"next_obs"``) state:
    ``linear`` w x, ``square`` w x^2, ``abs`` w |x|, ``inside`` w [lo < x < hi], ``outside`` w ([x > hi] + [x < lo]);
    plus ``ctrl_cost`` c (- c sum a^2) and a constant ``bonus``.
The step reward is evaluated as ``((terms of the first term's dim pair) - c ctrl) + bonus``, then the other terms: with that order
the built-in halfcheetah, ant and slim humanoid closures restate bit for bit (tests/test_env_spec.py).

How a spec is found: ``envs.resolve_env_kind`` follows an env's ``wrapped_env`` chain for an explicit ``cadm_env_spec`` attribute
(an ``EnvDecl`` is its own).  Nothing is inferred from an env's duck type.
"""
import hashlib
import json
import math

import numpy as np

# kernels' envelope (include/cadm_hip.h CADM_SPEC_MAX_*): the head fits one 8-dim tile per wave (D <= 64) and the state of a row
# two pair slots per thread; the bounds below are what the layouts were checked at (slim humanoid's (45, 17, 45) inside)
MAX_D, MAX_A, MAX_P, MAX_TERMS = 48, 24, 64, 32
PRE = {"id": 0, "drop": 1, "sincos": 2}
POST = {"add": 0, "replace": 1}
TERMS = {"linear": 0, "square": 1, "abs": 2, "inside": 3, "outside": 4}
WHEN = {"obs": 0, "next_obs": 1}
ENV_KIND_SPEC = 5          # CADM_ENV_SPEC
_FEATS = {(): "drop", ("id",): "id", ("sin", "cos"): "sincos"}


class _Box:
    def __init__(self, dim):
        self.shape = (dim,)
        self.low = -np.ones(dim)
        self.high = np.ones(dim)


def _f32(x):
    return float(np.float32(x))


def _canon_pre(d, e):
    if isinstance(e, str):
        if e not in PRE:
            raise ValueError("preproc[%d] = %r: expected one of %s" % (d, e, sorted(PRE)))
        return e
    feats = tuple(e)
    if len(feats) > 2:
        raise ValueError("preproc[%d] yields %d features %r: an obs dim feeds at most 2 features (the kernels' dim_feats)"
                         % (d, len(feats), feats))
    if feats not in _FEATS:
        raise ValueError("preproc[%d] = %r: the features of one dim are (), ('id',) or ('sin', 'cos')" % (d, feats))
    return _FEATS[feats]


class EnvDecl:
    """A user-declared env: spaces, the four numpy closures and what the library compiles from them.

    >>> EnvDecl(obs_dim=3, act_dim=1, preproc=["sincos", "id", "id"], postproc="add",
    ...         reward=[dict(kind="square", dim=2, w=-0.1)], ctrl_cost=0.001)
    """

    def __init__(self, obs_dim, act_dim, preproc="id", postproc="add", reward=(), ctrl_cost=0.0, bonus=0.0):
        D, A = int(obs_dim), int(act_dim)
        if not 1 <= D <= MAX_D:
            raise ValueError("obs_dim D=%d outside the kernels' envelope 1 <= D <= %d" % (D, MAX_D))
        if not 1 <= A <= MAX_A:
            raise ValueError("act_dim A=%d outside the kernels' envelope 1 <= A <= %d" % (A, MAX_A))
        pre = [preproc] * D if isinstance(preproc, str) else list(preproc)
        post = [postproc] * D if isinstance(postproc, str) else list(postproc)
        if len(pre) != D or len(post) != D:
            raise ValueError("preproc / postproc need one entry per obs dim (D=%d), got %d / %d" % (D, len(pre), len(post)))
        pre = [_canon_pre(d, e) for d, e in enumerate(pre)]
        for d, e in enumerate(post):
            if e not in POST:
                raise ValueError("postproc[%d] = %r: expected one of %s" % (d, e, sorted(POST)))
        P = sum({"id": 1, "drop": 0, "sincos": 2}[e] for e in pre)
        if not 1 <= P <= MAX_P:
            raise ValueError("preproc yields P=%d features, outside the kernels' envelope 1 <= P <= %d" % (P, MAX_P))
        terms = []
        for k, t in enumerate(reward):
            t = dict(t)
            kind, dim, when = t.pop("kind"), int(t.pop("dim")), t.pop("when", "obs")
            w, lo, hi = float(t.pop("w", 1.0)), t.pop("lo", None), t.pop("hi", None)
            if t:
                raise ValueError("reward term %d: unknown field(s) %s" % (k, sorted(t)))
            if kind not in TERMS:
                raise ValueError("reward term %d: kind %r, expected one of %s" % (k, kind, sorted(TERMS)))
            if when not in WHEN:
                raise ValueError("reward term %d: when %r, expected one of %s" % (k, when, sorted(WHEN)))
            if not 0 <= dim < D:
                raise ValueError("reward term %d reads obs dim %d, outside 0 .. D-1 = %d" % (k, dim, D - 1))
            if kind in ("inside", "outside"):
                if lo is None or hi is None or not float(lo) < float(hi):
                    raise ValueError("reward term %d (%s) needs lo < hi, got lo=%r hi=%r" % (k, kind, lo, hi))
                lo, hi = float(lo), float(hi)
            elif lo is not None or hi is not None:
                raise ValueError("reward term %d (%s) takes no lo / hi" % (k, kind))
            else:
                lo = hi = 0.0
            for v in (w, lo, hi):
                if not math.isfinite(v) or not math.isfinite(_f32(v)):
                    raise ValueError("reward term %d: non-finite (or beyond float32) constant %r" % (k, v))
            terms.append((kind, dim, when, w, lo, hi))
        if len(terms) > MAX_TERMS:
            raise ValueError("%d reward terms, at most %d" % (len(terms), MAX_TERMS))
        ctrl_cost, bonus = float(ctrl_cost), float(bonus)
        if not (math.isfinite(_f32(ctrl_cost)) and math.isfinite(_f32(bonus))):
            raise ValueError("ctrl_cost / bonus must be finite float32 numbers")
        self.obs_dim, self.act_dim, self.proc_obs_dim = D, A, P
        self.preproc, self.postproc, self.terms = tuple(pre), tuple(post), tuple(terms)
        self.ctrl_cost, self.bonus = ctrl_cost, bonus
        # the reference env's duck type (dynamics.py:185-187)
        self.observation_space = _Box(D)
        self.action_space = _Box(A)
        self.proc_observation_space_dims = P
        self.cadm_env_spec = self
        self._src = [d for d, e in enumerate(pre) for _ in range({"id": 1, "drop": 0, "sincos": 2}[e])]
        self._op = [o for e in pre for o in {"id": ("id",), "drop": (), "sincos": ("sin", "cos")}[e]]
        self._replace = np.array([e == "replace" for e in post])
        self.canonical = self._canonical()
        self.hash = hashlib.sha256(self.canonical.encode()).hexdigest()
        self.hash64 = int(self.hash[:16], 16)

    # ------------------------------------------------------------------ identity
    def _canonical(self):
        """Canonical serialisation: every field, floats as the exact hex of their float64 value.  Equal specs serialise equally."""
        return json.dumps({"version": 1, "obs_dim": self.obs_dim, "act_dim": self.act_dim, "preproc": list(self.preproc),
                           "postproc": list(self.postproc),
                           "reward": [[k, d, w, wt.hex(), lo.hex(), hi.hex()] for (k, d, w, wt, lo, hi) in self.terms],
                           "ctrl_cost": self.ctrl_cost.hex(), "bonus": self.bonus.hex()}, sort_keys=True, separators=(",", ":"))

    @property
    def hash_words(self):
        """(low, high) 32-bit words of the 64-bit spec hash, as the signed ints of cadm_config.reserved[0..1]."""
        lo, hi = self.hash64 & 0xFFFFFFFF, self.hash64 >> 32
        return tuple(int(np.array(v, np.uint32).view(np.int32)) for v in (lo, hi))

    def __eq__(self, other):
        return isinstance(other, EnvDecl) and other.canonical == self.canonical

    def __hash__(self):
        return self.hash64

    def __repr__(self):
        return "EnvDecl(D=%d, A=%d, P=%d, %d reward terms, hash %s)" % (self.obs_dim, self.act_dim, self.proc_obs_dim, len(self.terms),
                                                                       self.hash[:16])

    # ------------------------------------------------------------------ what the library compiles
    def header(self):
        """The generated cadm_spec_tables.h of a rollout module (cadm_amd/jit.py): data tables only, read by csrc/env_tables.h."""
        def fl(x):
            return float(np.float32(x)).hex() + "f"

        def mask(pred):
            return "0x%016xull" % sum(1 << d for d in range(self.obs_dim) if pred(d))
        terms = "".join("{%d, %d, %d, %s, %s, %s}, " % (TERMS[k], d, WHEN[w], fl(wt), fl(lo), fl(hi)) for (k, d, w, wt, lo, hi) in self.terms)
        lo, hi = self.hash64 & 0xFFFFFFFF, self.hash64 >> 32
        return "\n".join([
            "// generated by cadm_amd/env_spec.py from env spec %s -- data tables only" % self.hash[:16],
            "#pragma once",
            "#define CADM_SPEC_HASH_LO 0x%08xu" % lo,
            "#define CADM_SPEC_HASH_HI 0x%08xu" % hi,
            "#define CADM_SPEC_D %d" % self.obs_dim,
            "#define CADM_SPEC_A %d" % self.act_dim,
            "#define CADM_SPEC_P %d" % self.proc_obs_dim,
            "#define CADM_SPEC_DROP_MASK %s" % mask(lambda d: self.preproc[d] == "drop"),
            "#define CADM_SPEC_SINCOS_MASK %s" % mask(lambda d: self.preproc[d] == "sincos"),
            "#define CADM_SPEC_REPLACE_MASK %s" % mask(lambda d: self.postproc[d] == "replace"),
            "#define CADM_SPEC_NTERMS %d" % len(self.terms),
            "#define CADM_SPEC_TERMS %s" % terms,
            "#define CADM_SPEC_CTRL %s" % fl(self.ctrl_cost),
            "#define CADM_SPEC_BONUS %s" % fl(self.bonus),
            ""])

    def to_c(self):
        """The spec as include/cadm_hip.h's cadm_env_spec (for cadm_set_env_spec)."""
        from . import _lib
        s = _lib.EnvSpecC()
        s.obs_dim, s.act_dim, s.proc_obs_dim = self.obs_dim, self.act_dim, self.proc_obs_dim
        for d in range(self.obs_dim):
            s.preproc[d], s.postproc[d] = PRE[self.preproc[d]], POST[self.postproc[d]]
        s.n_terms = len(self.terms)
        for k, (kind, d, when, w, lo, hi) in enumerate(self.terms):
            s.term_kind[k], s.term_dim[k], s.term_when[k] = TERMS[kind], d, WHEN[when]
            s.term_w[k], s.term_lo[k], s.term_hi[k] = w, lo, hi
        s.ctrl_cost, s.bonus = self.ctrl_cost, self.bonus
        s.hash_lo, s.hash_hi = self.hash64 & 0xFFFFFFFF, self.hash64 >> 32
        return s

    # ------------------------------------------------------------------ closures (numpy, dtype-preserving)
    def obs_preproc(self, obs):
        parts = []
        for d, op in zip(self._src, self._op):
            x = obs[..., d:d + 1]
            parts.append(x if op == "id" else np.sin(x) if op == "sin" else np.cos(x))
        return np.concatenate(parts, axis=-1)

    def obs_postproc(self, obs, pred):
        return np.where(self._replace, pred, obs + pred)

    def targ_proc(self, obs, next_obs):
        return np.where(self._replace, next_obs, next_obs - obs)

    def _term(self, kind, x, w, lo, hi):
        dt = x.dtype.type
        if kind == "linear":
            return dt(w) * x
        if kind == "square":
            return dt(w) * (x * x)
        if kind == "abs":
            return dt(w) * np.abs(x)
        if kind == "inside":
            return np.where(np.logical_and(x > dt(lo), x < dt(hi)), dt(w), dt(0))
        return dt(w) * ((x > dt(hi)).astype(x.dtype) + (x < dt(lo)).astype(x.dtype))

    def reward(self, obs, act, next_obs):
        """Step reward (the kernels' grouping): ((terms of the first term's dim pair, pre-step) - c sum a^2) + bonus, then the others."""
        dt = obs.dtype.type
        first_pair = self.terms[0][1] >> 1 if self.terms else 0
        head = [k for k, t in enumerate(self.terms) if t[1] >> 1 == first_pair and t[2] == "obs"]
        r = None
        for k in head:
            kind, d, when, w, lo, hi = self.terms[k]
            v = self._term(kind, obs[..., d], w, lo, hi)
            r = v if r is None else r + v
        if r is None:
            r = np.zeros(obs.shape[:-1], obs.dtype)
        if self.ctrl_cost != 0.0:
            r = r - dt(self.ctrl_cost) * np.sum(np.square(act), axis=-1)
        if self.bonus != 0.0:
            r = r + dt(self.bonus)
        for k, (kind, d, when, w, lo, hi) in enumerate(self.terms):
            if k in head:
                continue
            r = r + self._term(kind, (obs if when == "obs" else next_obs)[..., d], w, lo, hi)
        return r


def restate(kind):
    """The built-in kinds halfcheetah, ant and slim humanoid as specs: tests, tools, and the closures of envs.EnvSpec.  The library
    keeps their hand-written kernels (profiles/env_tables_ab.md)."""
    if kind in ("halfcheetah", "cripple_halfcheetah"):      # half_cheetah_env.py:46-59,82-88
        return EnvDecl(18, 6, preproc=["drop", "id", "sincos"] + ["id"] * 15, postproc=["replace"] + ["add"] * 17,
                       reward=[dict(kind="linear", dim=0)], ctrl_cost=0.1)
    if kind == "ant":                                        # ant_env.py:52-62,89-98
        return EnvDecl(28, 8, preproc=["drop"] + ["id"] * 27, postproc=["replace"] + ["add"] * 27,
                       reward=[dict(kind="linear", dim=0)], ctrl_cost=0.005, bonus=0.05)
    if kind == "slim_humanoid":                              # slim_humanoid_env.py:39-46,95-111
        return EnvDecl(45, 17, reward=[dict(kind="linear", dim=22, w=0.25 / 0.015),
                                       dict(kind="inside", dim=1, w=5.0, lo=1.0, hi=2.0)], ctrl_cost=0.1)
    raise ValueError("no spec restatement of env kind %r" % (kind,))
