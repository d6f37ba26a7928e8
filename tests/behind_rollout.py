"""Inputs for the kernels behind the rollout (csrc/forecast.hip, csrc/constrain.hip) on the built-in kinds other than halfcheetah --
test infrastructure shared by tests/test_forecast_ref.py (CPU) and tests/test_gpu_behind_rollout_envs.py.

kind           engine p, H   synthetic m, n   rows                      seed   constrained dims, band
ant            10, 5         3, 7             210: 64, 64, 64, 18       21     (0, 27), mean +- 1.8 std
slim_humanoid  15, 3         2, 5             150: 64, 64, 22           22     (1, 44), mean +- 1.5 std
pendulum       5, 5          3, 9             135: 64, 64, 7            23     (2, 0),  mean +- 1.8 std

ant: p * D = 280 > 256, step spans always 16-byte aligned.  slim_humanoid: an odd D, spans aligned at even steps only, the largest
terminate-mode tiles of any built-in kind.  pendulum: D = 3, spans of mixed alignment."""
import numpy as np

KINDS = {      # kind: (D, A, engine p, H, m, n, seed, constrained dims, band width in std)
    "ant": (28, 8, 10, 5, 3, 7, 21, (0, 27), 1.8),
    "slim_humanoid": (45, 17, 15, 3, 2, 5, 22, (1, 44), 1.5),
    "pendulum": (3, 1, 5, 5, 3, 9, 23, (2, 0), 1.8),
}
HALFCHEETAH_B = (2, 8, 2, 1, 20, 18, 6)      # tests/test_gpu_forecast.py's shape (b): synth_traj's arguments

# The engines of tests/test_gpu_terms_envelope.py -- the planner terms behind the rollout (uncertainty, tracking, actuator, knots, value
# and reward nets) off the geometries their own files run on; the CPU tests of the restatements read the shapes from here.
TERM_ENGINES = {      # name: (env, D, A, E, p, H); "widest" is helpers.corner_spec's declaration, the others are built-in kinds
    "pend": ("pendulum", 3, 1, 5, 5, 5),
    "ant": ("ant", 28, 8, 5, 10, 5),
    "slim": ("slim_humanoid", 45, 17, 5, 15, 3),
    "slim35": ("slim_humanoid", 45, 17, 5, 35, 3),
    "wide": ("widest", 48, 24, 5, 10, 3),
    "long": ("halfcheetah", 18, 6, 5, 5, 40),
    "one": ("halfcheetah", 18, 6, 5, 5, 1),
    "p1": ("halfcheetah", 18, 6, 1, 1, 5),
}

# tests/test_gpu_critic_envelope.py runs the Q critics' kernel on seven of them, kernel level (nothing is rolled out); tests/test_critic_ref.py
# reads the shapes from here.  name: the (m, n) of its two launches -- KINDS' own where the kind has one, (3, 11) elsewhere, and one
# candidate of one env: fewer than 16 rows.  Rows at the engine's p: pend 135 = 8 x 16 + 7 and 5, ant 210 = 13 x 16 + 2 and 10, slim
# 150 = 9 x 16 + 6 and 15, wide 330 = 20 x 16 + 10 and 10, long and one 165 = 10 x 16 + 5 and 5, p1 33 = 2 x 16 + 1 and 1: every launch
# ends in a partial tile.
CRITIC_ROWS = {
    "pend": [KINDS["pendulum"][4:6], (1, 1)], "ant": [KINDS["ant"][4:6], (1, 1)], "slim": [KINDS["slim_humanoid"][4:6], (1, 1)],
    "wide": [(3, 11), (1, 1)], "long": [(3, 11), (1, 1)], "one": [(3, 11), (1, 1)], "p1": [(3, 11), (1, 1)],
}
CRITIC_GAMMA = 0.97      # "long": the discount the ctx carries, so that the row update multiplies by weight * disc[40]
# "long": the seed of the poisoned rows and the `first` cuts of the non-finite test.  Of 165 rows with `first` drawn over 0 .. 40 about
# four stay uncut; under the feature file's seed 13 none of them is a poisoned row, under 17 two poisoned and five clean ones are
# (the draws are numpy's and do not depend on the device; the test asserts the condition before it launches).
CRITIC_LONG_SEED = 17

# The engines of tests/test_gpu_policy_envelope.py -- the policy prior's roll and the guided loop off halfcheetah at p in {5, 20}, H <= 5;
# tests/test_policy_ref.py reads the shapes, the nets and the noise levels from here and shows on the CPU that the restatement alone
# meets the conditions the GPU tests put on their inputs.  Every built-in kind at hidden 200 x 4 and swish (nothing is built on demand),
# the problems as TERM_ENGINES' (m = 2, seed 3, `trained_like`; "wide": seed 8), widened to more envs by `with_rows`.
POLICY_ENGINES = {      # name: (env, D, A, E, p, H) + (context, (lower_bound, upper_bound) or None)
    "pend": TERM_ENGINES["pend"] + (True, None),                       # A = 1, D4 = 4
    "ant": ("ant", 28, 8, 5, 10, 3, True, None),                       # two full noise groups, p = 10
    "slim": TERM_ENGINES["slim"] + (True, None),                       # odd D, groups 0 .. 4 with one dim in the last, p = 15
    "long": TERM_ENGINES["long"] + (False, None),                      # H = 40: the CPU roll of tests/test_policy_ref.py stays finite over all 40
    "big": ("halfcheetah", 18, 6, 5, 5, 2, False, None),               # "long"'s weights: the roll with two row tiles per workgroup
    "bnd": ("halfcheetah", 18, 6, 5, 5, 3, True, (-0.5, 2.0)),         # bounds that are not -1, 1
    "wide": ("widest", 48, 24, 5, 10, 1, True, None),                  # noise at A = 24; H = 1: no rollout, no module built on demand
    "fit": ("halfcheetah", 18, 6, 5, 5, 5, False, None),               # tests/test_gpu_policy.py's "hc5-vanilla": the exact fit of the slots
}
POLICY_NET = ((50, 30, 70, 18), "swish", "tanh")      # tests/test_gpu_policy.py's net of the roll: `policy_ref.envelope_policy`
POLICY_BIG_NET = ((64, 48, 200), "swish", "tanh", 21)      # hidden, act, squash, `policy_ref.he_policy`'s seed (out_scale 0.5)
POLICY_BND_NET = ((37,) * 4, "tanh", 5, 1.0)      # hidden, act, `he_policy`'s seed and out_scale: with squash "none" both bounds are reached
POLICY_LOOP_NET = ((50, 30), "tanh", "tanh", 40)      # the guided loop's: hidden, act, squash, `he_policy`'s seed (out_scale 0.5)
POLICY_LONG_IN_SCALE = 2.0 ** -7      # "long": what the first layer of POLICY_NET is scaled by (`policy_layers`)
POLICY_SEED, POLICY_CALL = 5, 9
POLICY_ROLLS = {      # name: (noise_std, [(m, P)]) of `check_roll`
    "pend": (0.3, [(3, 6), (1, 17)]), "ant": (0.3, [(3, 6), (1, 17)]), "slim": (0.3, [(3, 6), (1, 17)]),
    "long": (0.2, [(2, 6)]), "big": (0.3, [(65, 127)]), "bnd": (0.5, [(3, 6)]), "wide": (0.25, [(3, 17)]),
}


def with_rows(prob, m, seed=77):
    """a copy of a synth problem with obs, cp_obs and cp_act grown to m envs: the problem's own rows first, then rows drawn as
    `synth.make_problem` draws them"""
    have = prob["obs"].shape[0]
    if m <= have:
        return dict(prob, obs=prob["obs"][:m], cp_obs=prob["cp_obs"][:m], cp_act=prob["cp_act"][:m], m=m)
    rng = np.random.default_rng(seed)
    D, A, Hh = prob["D"], prob["A"], prob["Hh"]
    more = m - have
    return dict(prob, m=m, obs=np.concatenate([prob["obs"], rng.standard_normal((more, D))]),
                cp_obs=np.concatenate([prob["cp_obs"], 0.1 * rng.standard_normal((more, D * Hh))]),
                cp_act=np.concatenate([prob["cp_act"], rng.uniform(-1.0, 1.0, (more, A * Hh))]))


def policy_problem(name, env=None):
    """the synth problem of one of POLICY_ENGINES (m = 2); env: the declaration behind "widest" (helpers.corner_spec), which this
    module does not import"""
    from cadm_amd import synth
    kind, D, A, E, p, H, context, _ = POLICY_ENGINES[name]
    if name == "wide":
        return synth.make_problem(env=env, context=True, E=E, m=2, H=H, seed=8)
    return synth.make_problem(env=kind, context=context, E=E, m=2, H=H, seed=3, trained_like=True)


def policy_layers(name, squash="tanh"):
    """(layers, act, squash) of the net tests/test_gpu_policy_envelope.py rolls on engine `name`.  "long": the synthetic model's states
    double every five steps (tests/test_policy_ref.py), so the first layer is scaled by 2^-7 -- an exact scaling -- and the tanh squash
    stays open over all 40; "wide": tests/test_gpu_policy.py's bias-only net of the noise test."""
    import policy_ref as pref
    _, D, A = POLICY_ENGINES[name][:3]
    if name == "wide":
        return [(np.zeros((D, A), np.float32), np.linspace(-0.3, 0.3, A).astype(np.float32))], "relu", "none"
    if name == "big":
        hidden, act, squash, seed = POLICY_BIG_NET
        return pref.he_policy(D, hidden, A, seed, 0.5), act, squash
    if name == "bnd":
        hidden, act, seed, scale = POLICY_BND_NET
        return pref.he_policy(D, hidden, A, seed, scale), act, squash
    hidden, act, squash = POLICY_NET
    layers = pref.envelope_policy(D, hidden, A)
    if name == "long":
        layers[0] = ((layers[0][0] * np.float32(POLICY_LONG_IN_SCALE)).astype(np.float32), layers[0][1])
    return layers, act, squash


def term_traj(name, m, n, seed):
    """`synth_traj` at the shape of one of TERM_ENGINES"""
    _, D, A, _, p, H = TERM_ENGINES[name]
    return synth_traj(seed, H, m, n, p, D, A)


def synth_traj(seed, H, m, n, p, D, A):
    """(traj [H,m,n,p,D], obs [m,D], actions [m,n,H,A]) float32: per-dim scales 0.5 .. 3 and offsets of order 1."""
    rng = np.random.default_rng(seed)
    traj = (rng.standard_normal((H, m, n, p, D)) * rng.uniform(0.5, 3.0, D) + rng.standard_normal(D)).astype(np.float32)
    return traj, rng.standard_normal((m, D)).astype(np.float32), rng.uniform(-1, 1, (m, n, H, A)).astype(np.float32)


def band(traj, d, k, lower_only=False):
    """dim d inside mean +- k std of that dim over the array (lower_only: above mean - k std)"""
    mu, sd = float(traj[..., d].mean()), float(traj[..., d].std())
    return dict(dim=d, lo=mu - k * sd) if lower_only else dict(dim=d, lo=mu - k * sd, hi=mu + k * sd)


def alive_share(traj, obs):
    """slim_humanoid: the share of PRE-step states (obs at step 0, traj[t - 1] after) whose dim 1 lies inside (1, 2)"""
    H, m, n, p, _ = traj.shape
    pre1 = np.concatenate([np.broadcast_to(obs[None, :, None, None, 1], (1, m, n, p)), traj[:-1, ..., 1]], axis=0)
    return float(((pre1 > np.float32(1.0)) & (pre1 < np.float32(2.0))).mean())


def kind_inputs(kind):
    """(traj, obs, actions, constraints) of one kind, with the adjustments that make its reward terms bite:
    slim_humanoid -- dim 1 redrawn around the alive bonus's interval (1, 2), two observations inside / outside it;
    pendulum -- actions scaled by 3 (a third of them beyond the torque clip at +-2), pre-step states planted exactly on atan2's
    branch cut, (x, y) = (-1, +0.0) and (-1, -0.0), and at its origin (0, 0)."""
    D, A, p, H, m, n, seed, dims, k = KINDS[kind]
    traj, obs, acts = synth_traj(seed, H, m, n, p, D, A)
    if kind == "slim_humanoid":
        traj[..., 1] = (1.5 + 0.5 * np.random.default_rng(99).standard_normal(traj.shape[:-1])).astype(np.float32)
        obs[:2, 1] = [1.2, 2.3]
        assert 0.2 <= alive_share(traj, obs) <= 0.8, "slim_humanoid: alive share %.2f" % alive_share(traj, obs)
    if kind == "pendulum":
        acts = (acts * np.float32(3.0)).astype(np.float32)
        assert (np.abs(acts) > 2.0).mean() > 0.1, "pendulum: %.2f of the actions are clipped" % (np.abs(acts) > 2.0).mean()
        obs[0, :2] = [-1.0, 0.0]                 # step 0's pre-step state of env 0: theta = +pi
        traj[0, 1, 0, 0, :2] = [-1.0, -0.0]      # step 1's pre-step state of row (1, 0, 0): theta = -pi
        traj[1, 2, 0, 1, :2] = [0.0, 0.0]        # step 2's pre-step state of row (2, 0, 1): atan2(0, 0) = 0
    return traj, obs, acts, [band(traj, d, k) for d in dims]
