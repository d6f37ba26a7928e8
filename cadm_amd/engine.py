"""HipEngine: device state (weights, stats, scratch) + typed calls into libcadm_hip.so.

PyTorch-ROCm is used for device memory, the current HIP stream and (for multi-GPU)
torch.distributed only; every planner / training FLOP runs in the hand-written HIP
kernels behind the C ABI.  No host fallback exists: without a GPU or without the
built library the constructor raises.
"""
import ctypes as ct
import math
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._lib import Config, TrainHParams, check, ptr

STAT_KEYS = ("obs_mean", "obs_std", "act_mean", "act_std", "delta_mean", "delta_std",
             "cp_obs_mean", "cp_obs_std", "cp_act_mean", "cp_act_std",
             "back_delta_mean", "back_delta_std")


def dyn_param_names(n_hidden):
    """tf.trainable_variables() creation order inside one dynamics MLP
    (/root/reference/cadm/dynamics/core/utils.py:313-339)."""
    names = []
    for i in range(n_hidden):
        names += ["hidden_%d_weight" % i, "hidden_%d_bias" % i]
    names += ["output_mu_weight", "output_mu_bias", "output_logvar_weight", "output_logvar_bias",
              "max_logvar", "min_logvar"]
    return names


def ctx_param_names(n_cp_hidden):
    """core/utils.py:595-612."""
    names = []
    for i in range(n_cp_hidden):
        names += ["cp_hidden_%d_weight" % i, "cp_hidden_%d_bias" % i]
    return names + ["cp_output_weight", "cp_output_bias"]


# The nest of the opt-in loop's entry points, inner to outer.  Per level: the method (its export is cadm_<method>); what that export takes
# in front of the level below's arguments, in its order -- the method takes the same but "update" (read off the params) and "T" (read off
# the targets) --; and, for a level with workspace slots of its own, the slot's tag and how many of (terminate, actuator, uncertainty, P)
# key the slot and size it (cadm_<level>_workspace_bytes).  The levels without a tag share the slots `_loop_workspace` names by what they
# are given.  From `actuated_plan` outwards a level whose own struct (its first argument) is None hands the call to the level below.
# A further term is one row here and one public method of one call; in the library, one export and one field of PlanTerms.
_PLAN_NEST = (
    ("scored_plan", ("score", "update", "params"), None, 0),
    ("constrained_plan", ("constraints",), None, 0),
    ("knot_plan", ("knots", "phase"), None, 0),
    ("tracking_plan", ("track", "targets", "T", "offset"), None, 0),
    ("actuated_plan", ("actuator", "prev", "prefix", "advance"), None, 0),
    ("uncertain_plan", ("uncertainty",), "unc", 2),
    ("valued_plan", ("value",), "val", 3),
    ("rewarded_plan", ("reward",), "rew", 3),
    ("guided_plan", ("policy",), "pol", 4),
    ("critic_plan", ("critic",), "crt", 4),
    ("anchored_plan", ("logp",), "anc", 4),
)
_PLAN_LEVEL = {row[0]: i for i, row in enumerate(_PLAN_NEST)}
# how many arguments each level's export takes between ctx and obs, and each level's method in front of obs
_PLAN_NHEAD = [sum(len(row[1]) for row in _PLAN_NEST[:i + 1]) for i in range(len(_PLAN_NEST))]
_PLAN_NARGS = [sum(len(set(row[1]) - {"update", "T"}) for row in _PLAN_NEST[:i + 1]) for i in range(len(_PLAN_NEST))]
# outer to inner: (method, where its own struct stands in the outermost method's arguments); (slot tag, size export) of the levels with one
_PLAN_ROUTES = tuple((row[0], -n) for row, n in zip(reversed(_PLAN_NEST), reversed(_PLAN_NARGS)))
_PLAN_SLOTS = tuple((row[2], "cadm_%s_workspace_bytes" % row[0][:-len("_plan")]) for row in reversed(_PLAN_NEST) if row[2])
_KNOT, _ACTUATED = _PLAN_LEVEL["knot_plan"], _PLAN_LEVEL["actuated_plan"]


def _by(struct):
    return None if struct is None else ct.byref(struct)


class HipEngine:
    def __init__(self, env_kind, E, p, D, A, P, C, hidden_sizes, H, deterministic=False, discrete=False,
                 reference_quirks=True, history_length=10, cp_hidden_sizes=(256, 128, 64), back_model=False,
                 num_elites=50, num_cem_iters=5, alpha=0.1, lower_bound=-1.0, upper_bound=1.0, device=None, lib=None,
                 hidden_nonlinearity="swish"):
        if not torch.cuda.is_available():
            raise _lib.CadmError("no HIP device visible: the CaDM planner runs only on the GPU "
                                 "(libcadm_hip.so); there is no CPU fallback")
        # lib: a developer build (tests / tools: _lib.load_dev()); the product always binds libcadm_hip.so
        self.lib = lib if lib is not None else _lib.load()
        self._ext = None            # host-supplied all-gather of a sharded planner (dist_init_external)

        def _check(rc, what=""):
            # an exception raised inside the host-supplied collective cannot cross the library's C frames: re-raise it here
            ext = self._ext
            if rc and ext is not None and ext.error is not None:
                exc, ext.error = ext.error, None
                raise exc
            check(rc, what, self.lib)
        self._check = _check
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        hs = tuple(int(h) for h in hidden_sizes)
        if len(hs) < 1 or min(hs) < 1:
            raise ValueError("hidden_sizes must be positive, got %r" % (hs,))
        # Unequal hidden widths (the reference accepts any tuple, dynamics.py:28): the library works on ONE width, the widest
        # layer's, and the narrower layers are ZERO-PADDED to it -- a padded unit has zero weights and bias on both sides, so it
        # contributes nothing to any layer, its pre-activation is 0 and (for every nonlinearity with act(0) = 0) so is its
        # output: all its gradients are exactly 0, weight decay included, and Adam leaves an exact zero where it is.  The
        # padded tensors are what the library sees; `param_shapes_true` / `params_list` / `load_params_list` speak the model's
        # own shapes (checkpoints are the reference's).  sigmoid(0) = 0.5 would put gradient on the padded weights: refused.
        self.hidden_sizes = hs
        self._padded = len(set(hs)) != 1
        if self._padded and hidden_nonlinearity == "sigmoid":
            raise NotImplementedError("unequal hidden_sizes %r with hidden_nonlinearity='sigmoid': zero-padded units would train "
                                      "(sigmoid(0) != 0); use equal widths or swish / relu / tanh / None" % (hs,))
        # env_kind: a built-in kind name, or a user-declared env (env_spec.EnvDecl) whose closures the rollout module is built from
        from .env_spec import EnvDecl
        self.spec = env_kind if isinstance(env_kind, EnvDecl) else None
        if self.spec is not None and (D, A, P) != (self.spec.obs_dim, self.spec.act_dim, self.spec.proc_obs_dim):
            raise ValueError("env spec dims (D=%d, A=%d, P=%d) differ from the model's (D=%d, A=%d, P=%d)"
                             % (self.spec.obs_dim, self.spec.act_dim, self.spec.proc_obs_dim, D, A, P))
        if self.spec is not None and discrete:
            raise ValueError("env specs declare continuous actions only")
        self.env_kind, self.E, self.p, self.D, self.A, self.P, self.C = env_kind, E, p, D, A, P, C
        self.H, self.NH, self.HID = H, len(hs), max(hs)
        self.Hh = history_length
        self.cp_hidden_sizes = tuple(cp_hidden_sizes)
        self.deterministic, self.discrete = bool(deterministic), bool(discrete)
        self.back_model = bool(back_model)
        self.K0 = P + A + C
        if hidden_nonlinearity not in _lib.ACT_KINDS:
            raise NotImplementedError("hidden_nonlinearity %r: the kernels implement swish / relu / tanh / sigmoid / None" % (hidden_nonlinearity,))
        self.hidden_nonlinearity, self.hidden_act = hidden_nonlinearity, _lib.ACT_KINDS[hidden_nonlinearity]
        self._rollout_ready = set()
        cfg = Config()
        cfg.abi_version = _lib.ABI_VERSION
        if self.spec is not None:
            cfg.env_kind = _lib.ENV_SPEC
            cfg.reserved[0], cfg.reserved[1] = self.spec.hash_words
        else:
            cfg.env_kind = _lib.ENV_KINDS[env_kind]
        cfg.ensemble_size, cfg.n_particles = E, p
        cfg.obs_dim, cfg.act_dim, cfg.proc_obs_dim, cfg.context_dim = D, A, P, C
        cfg.n_hidden, cfg.hidden, cfg.horizon = self.NH, self.HID, H
        cfg.deterministic, cfg.discrete = int(self.deterministic), int(self.discrete)
        cfg.reference_quirks = int(bool(reference_quirks))
        cfg.history_length = history_length
        cfg.n_cp_hidden = len(self.cp_hidden_sizes) if C > 0 else 0
        for i, h in enumerate(self.cp_hidden_sizes if C > 0 else ()):
            cfg.cp_hidden[i] = int(h)
        cfg.num_elites, cfg.num_cem_iters, cfg.alpha = num_elites, num_cem_iters, alpha
        cfg.lower_bound, cfg.upper_bound = lower_bound, upper_bound
        cfg.back_model = int(self.back_model)
        cfg.hidden_act = self.hidden_act
        self.cfg = cfg
        self.num_elites, self.num_cem_iters = num_elites, num_cem_iters
        self._ctx = C_void_p()
        with torch.cuda.device(self.device):
            self._check(self.lib.cadm_ctx_create(ct.byref(cfg), ct.byref(self._ctx)), "cadm_ctx_create")
            if self.spec is not None:
                self._spec_c = self.spec.to_c()
                self._check(self.lib.cadm_set_env_spec(self._ctx, ct.byref(self._spec_c)), "cadm_set_env_spec")
        self.nets = OrderedDict()   # net name -> OrderedDict(param name -> tensor)
        self._ws = None
        self._ws_key = None
        self._host_plan = None
        self._loop_ws = {}          # the opt-in loop's workspaces: (mppi, with trajectory view) -> ((m, n, K), tensor)
        self._train_B = 0
        self.dist_world, self.dist_rank = 1, 0

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self.lib.cadm_ctx_destroy(self._ctx)
            self._ctx = C_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self):
        return ct.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _t(self, x, dtype=torch.float32):
        """numpy / tensor -> contiguous device tensor."""
        if isinstance(x, torch.Tensor):
            return x.to(device=self.device, dtype=dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(self.device)

    def stage(self, arrays):
        """Host arrays -> device tensors through ONE pinned staging buffer and ONE async H2D copy (the planner's
        per-call inputs are five tiny arrays; five pageable copies cost more than the copy itself).  None stays None."""
        live = [(i, np.asarray(a, dtype=np.float32)) for i, a in enumerate(arrays) if a is not None]
        total = sum(a.size for _, a in live)
        if getattr(self, "_stage_host", None) is None or self._stage_host.numel() < total:
            self._stage_host = torch.empty(max(total, 4096), dtype=torch.float32).pin_memory()
            self._stage_dev = torch.empty_like(self._stage_host, device=self.device)
        hv = self._stage_host.numpy()
        out, off = [None] * len(arrays), 0
        for i, a in live:
            hv[off:off + a.size] = a.reshape(-1)
            out[i] = (off, a.shape)
            off += a.size
        self._stage_dev[:off].copy_(self._stage_host[:off], non_blocking=True)
        return [None if o is None else self._stage_dev[o[0]:o[0] + int(np.prod(o[1]))].view(o[1]) for o in out]

    # ------------------------------------------------------------------ weights
    def net_names(self):
        names = []
        if self.C > 0:
            names.append("context_model")
        names.append("ff_model")
        if self.back_model:
            names.append("backward_model")
        return names   # = variable-scope creation order (dynamics.py:140,159,213)

    def param_shapes_true(self, net):
        """The model's own tensor shapes (the reference's checkpoint layout) -- differ from `param_shapes` (what the library
        holds) only for unequal hidden widths, which are zero-padded to the widest layer."""
        shapes = self.param_shapes(net)
        if net == "context_model" or not self._padded:
            return shapes
        E, hs = self.E, self.hidden_sizes
        sizes = [self.K0] + list(hs)
        for i in range(self.NH):
            shapes["hidden_%d_weight" % i] = (E, sizes[i], sizes[i + 1])
            shapes["hidden_%d_bias" % i] = (E, 1, sizes[i + 1])
        for head in ("output_mu", "output_logvar"):
            shapes[head + "_weight"] = (E, hs[-1], self.D)
        return shapes

    def _pad(self, net, name, arr):
        """Model-shaped array -> library-shaped (zero-padded) array; library-shaped input passes through."""
        want, true = self.param_shapes(net)[name], self.param_shapes_true(net)[name]
        a = np.asarray(arr) if not isinstance(arr, torch.Tensor) else arr
        if tuple(a.shape) == tuple(want) or tuple(a.shape) != tuple(true):
            return arr
        if isinstance(a, torch.Tensor):
            out = torch.zeros(want, dtype=a.dtype, device=a.device)
        else:
            out = np.zeros(want, dtype=a.dtype)
        out[tuple(slice(0, n) for n in true)] = a
        return out

    def param_shapes(self, net):
        E = self.E
        shapes = OrderedDict()
        if net == "context_model":
            sizes = [(self.D + self.A) * self.Hh] + list(self.cp_hidden_sizes)
            for i in range(len(sizes) - 1):
                shapes["cp_hidden_%d_weight" % i] = (E, sizes[i], sizes[i + 1])
                shapes["cp_hidden_%d_bias" % i] = (E, 1, sizes[i + 1])
            shapes["cp_output_weight"] = (E, sizes[-1], self.C)
            shapes["cp_output_bias"] = (E, 1, self.C)
        else:
            sizes = [self.K0] + [self.HID] * self.NH
            for i in range(self.NH):
                shapes["hidden_%d_weight" % i] = (E, sizes[i], sizes[i + 1])
                shapes["hidden_%d_bias" % i] = (E, 1, sizes[i + 1])
            for head in ("output_mu", "output_logvar"):
                shapes[head + "_weight"] = (E, self.HID, self.D)
                shapes[head + "_bias"] = (E, 1, self.D)
            shapes["max_logvar"] = (1, self.D)
            shapes["min_logvar"] = (1, self.D)
        return shapes

    def init_weights(self, rng):
        """Reference initialiser: trunc_normal(std = 1/(2 sqrt(in))), bias 0, logvar bounds 0.5 / -10
        (core/utils.py:338-339,636-641)."""
        for net in self.net_names():
            params = OrderedDict()
            for name, shape in self.param_shapes_true(net).items():      # (true fan-in for the initialiser; set_net pads)
                if name == "max_logvar":
                    v = np.ones(shape) / 2.0
                elif name == "min_logvar":
                    v = -np.ones(shape) * 10.0
                elif name.endswith("_bias"):
                    v = np.zeros(shape)
                else:
                    std = 1.0 / (2.0 * np.sqrt(shape[1]))
                    v = rng.standard_normal(shape)
                    bad = np.abs(v) > 2.0
                    while bad.any():
                        v[bad] = rng.standard_normal(int(bad.sum()))
                        bad = np.abs(v) > 2.0
                    v = v * std
                params[name] = v
            self.set_net(net, params)

    def set_net(self, net, params):
        """Install parameters (numpy or tensors) for one net and register them with the library."""
        shapes = self.param_shapes(net)
        cur = self.nets.get(net)
        out = OrderedDict()
        for name, shape in shapes.items():
            t = self._t(self._pad(net, name, params[name]))
            if tuple(t.shape) != tuple(shape):
                raise ValueError("%s/%s: shape %r != %r" % (net, name, tuple(t.shape), tuple(shape)))
            if cur is not None:     # keep registered device pointers stable
                cur[name].copy_(t)
                t = cur[name]
            out[name] = t
        self.nets[net] = out
        if cur is None:
            self._register(net)
        if cur is not None or net == "ff_model":     # weights rewritten in place: the library's packed copies follow
            if "ff_model" in self.nets:
                self._check(self.lib.cadm_repack(self._ctx, self.stream), "cadm_repack")

    def _register(self, net):
        prm = self.nets[net]
        nid = {"ff_model": _lib.NET_FF, "backward_model": _lib.NET_BACK, "context_model": _lib.NET_CTX}[net]
        if net == "context_model":
            layers = ["cp_hidden_%d" % i for i in range(len(self.cp_hidden_sizes))] + ["cp_output"]
        else:
            layers = ["hidden_%d" % i for i in range(self.NH)] + ["output_mu", "output_logvar"]
        for li, base in enumerate(layers):
            self._check(self.lib.cadm_set_weights(self._ctx, nid, li, ptr(prm[base + "_weight"]), ptr(prm[base + "_bias"])),
                  "cadm_set_weights")
        if net != "context_model":
            self._check(self.lib.cadm_set_logvar_bounds(self._ctx, nid, ptr(prm["max_logvar"]), ptr(prm["min_logvar"])),
                  "cadm_set_logvar_bounds")

    def repack(self):
        self._check(self.lib.cadm_repack(self._ctx, self.stream), "cadm_repack")

    def params_list(self):
        """Flat list of numpy arrays in the reference's tf.trainable_variables() order
        (context_model, ff_model, backward_model; dynamics.py:266)."""
        out = []
        for net in self.net_names():
            true = self.param_shapes_true(net)
            for name, t in self.nets[net].items():
                a = t.detach().cpu().numpy()
                out.append(a[tuple(slice(0, n) for n in true[name])].copy())      # (padding of unequal hidden widths stripped)
        return out

    def load_params_list(self, arrays):
        it = iter(arrays)
        for net in self.net_names():
            params = OrderedDict()
            for name in self.param_shapes(net):
                params[name] = np.asarray(next(it))
            self.set_net(net, params)

    # ------------------------------------------------------------------ stats
    def set_stats(self, stats):
        arrs = [np.ascontiguousarray(np.asarray(stats[k], dtype=np.float32)).reshape(-1) for k in STAT_KEYS]
        lens = [self.P, self.P, self.A, self.A, self.D, self.D, self.D * self.Hh, self.D * self.Hh,
                self.A * self.Hh, self.A * self.Hh, self.D, self.D]
        for k, a, n in zip(STAT_KEYS, arrs, lens):
            if a.size != n:
                raise ValueError("stat %s has %d entries, expected %d" % (k, a.size, n))
        ptrs = (ct.c_void_p * 12)(*[a.ctypes.data_as(ct.c_void_p) for a in arrs])
        self._check(self.lib.cadm_set_norm_stats(self._ctx, ptrs, self.stream), "cadm_set_norm_stats")

    # ------------------------------------------------------------------ rollout kernel for this geometry
    def ensure_rollout(self, noise=None, m=1, n_local=1):
        """The rollout kernel is compile-time specialised per geometry: make sure one exists for this engine (compiled in, or
        built on demand by cadm_amd.jit -- ~30 s the first time, cached) and that a launch fits the hardware (LDS for this
        horizon), so that a problem shows at construction, not at the first `get_action`."""
        from . import jit
        if noise is None:
            noise = _lib.NOISE_NONE if self.deterministic else _lib.NOISE_PHILOX
        if noise not in self._rollout_ready:
            jit.ensure(self, noise)
            self._check(self.lib.cadm_rollout_check(self._ctx, noise, int(m), int(n_local)), "cadm_rollout_check")
            self._rollout_ready.add(noise)

    # ------------------------------------------------------------------ planner primitives
    def context_forward(self, cp_obs, cp_act, bs=False):
        cp_obs, cp_act = self._t(cp_obs), self._t(cp_act)
        m = cp_obs.shape[1] if bs else cp_obs.shape[0]
        out = torch.empty((self.E, m, self.C), dtype=torch.float32, device=self.device)
        self._check(self.lib.cadm_context_forward(self._ctx, ptr(cp_obs), ptr(cp_act), m, int(bs), ptr(out), self.stream),
              "cadm_context_forward")
        return out

    def sample_actions(self, mean, var, n_global, z=None, seed=0, call=0, it=0, cand_offset=0, n_local=None):
        """Candidates [cand_offset, cand_offset + n_local) of the [m, n_global, H, A] buffer (default: all of them).  A rank of a sharded
        planner draws only its own shard -- the draws are keyed by the global element index -- and leaves the rest of the buffer alone."""
        mean, var = self._t(mean), self._t(var)
        m = mean.shape[0]
        z = None if z is None else self._t(z)
        n_local = n_global - cand_offset if n_local is None else n_local
        out = torch.empty((m, n_global, self.H, self.A), dtype=torch.float32, device=self.device)
        self._check(self.lib.cadm_sample_actions_shard(self._ctx, ptr(mean), ptr(var), ptr(z), seed, call, it, m, n_global, cand_offset,
                                                       n_local, ptr(out), self.stream), "cadm_sample_actions")
        return out

    def sample_uniform(self, m, n_global, seed=0, call=0):
        out = torch.empty((m, n_global, self.H, self.A), dtype=torch.float32, device=self.device)
        raw = torch.empty((m, n_global, self.H), dtype=torch.int32, device=self.device) if self.discrete else None
        self._check(self.lib.cadm_sample_uniform(self._ctx, seed, call, m, n_global, ptr(out), ptr(raw), self.stream),
              "cadm_sample_uniform")
        return out, raw

    def rollout_returns(self, obs, ctx_vec, actions, eps=None, obs_rows=None, norm_actions=True, seed=0, call=0,
                        it=0, cand_offset=0, n_local=None, want_traj=False):
        obs, actions = self._t(obs), self._t(actions)
        m, n_global = actions.shape[0], actions.shape[1]
        n_local = n_global - cand_offset if n_local is None else n_local
        ctx_vec = None if ctx_vec is None else self._t(ctx_vec)
        eps = None if eps is None else self._t(eps)
        obs_rows = None if obs_rows is None else self._t(obs_rows)
        self.ensure_rollout(_lib.NOISE_NONE if self.deterministic else _lib.NOISE_INJECT if eps is not None else _lib.NOISE_PHILOX, m, n_local)
        rows = torch.empty((m, n_local, self.p), dtype=torch.float32, device=self.device)
        traj = (torch.empty((self.H, m, n_local, self.p, self.D), dtype=torch.float32, device=self.device)
                if want_traj else None)
        self._check(self.lib.cadm_rollout_returns(self._ctx, ptr(obs), ptr(obs_rows), ptr(ctx_vec), ptr(actions), ptr(eps),
                                            int(norm_actions), seed, call, it, cand_offset, n_global, m, n_local,
                                            ptr(rows), ptr(traj), self.stream), "cadm_rollout_returns")
        return (rows, traj) if want_traj else rows

    def particle_mean(self, rows):
        m, n_local = rows.shape[0], rows.shape[1]
        out = torch.empty((m, n_local), dtype=torch.float32, device=self.device)
        self._check(self.lib.cadm_particle_mean(self._ctx, ptr(rows), m, n_local, ptr(out), self.stream), "cadm_particle_mean")
        return out

    def cem_refit(self, cand, actions, mean, var, G=1, want_elites=False, regen=None):
        """cand [G,m,n_local] (or [m,n] when G == 1); mean/var updated IN PLACE.  regen = (seed, call, it): the elites' action
        sequences are drawn again from the device RNG by global candidate id instead of being read from `actions` (a rank of a
        sharded planner holds only its own shard's draws); bit-identical to the gathered form."""
        m = actions.shape[0]
        n_local = actions.shape[1] // G
        el = torch.empty((m, self.num_elites), dtype=torch.int32, device=self.device) if want_elites else None
        if regen is not None:
            seed, call, it = regen
            self._check(self.lib.cadm_cem_refit_regen(self._ctx, ptr(cand), G, n_local, m, ptr(mean), ptr(var), seed, call, it, ptr(el),
                                                      self.stream), "cadm_cem_refit_regen")
            return el
        self._check(self.lib.cadm_cem_refit(self._ctx, ptr(cand), G, n_local, ptr(actions), m, ptr(mean), ptr(var), ptr(el),
                                      self.stream), "cadm_cem_refit")
        return el

    def rs_select(self, cand, actions, G=1):
        m = actions.shape[0]
        n_local = actions.shape[1] // G
        out = torch.empty((m, self.A), dtype=torch.float32, device=self.device)
        best = torch.empty((m,), dtype=torch.int32, device=self.device)
        self._check(self.lib.cadm_rs_select(self._ctx, ptr(cand), G, n_local, ptr(actions), m, ptr(out), ptr(best),
                                      self.stream), "cadm_rs_select")
        return out, best

    # ------------------------------------------------------------------ fused planners
    def _workspace(self, m, n):
        key = (m, n)
        if self._ws_key != key:
            nbytes = self.lib.cadm_plan_workspace_bytes(self._ctx, m, n)
            self._ws = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
            self._ws_key = key
            self._host_plan = None          # (holds a pointer into the workspace)
        return self._ws

    def host_out(self, shape):
        """Persistent PINNED host buffer the planners can write their (tiny) result into directly: the last kernel of a plan
        stores over PCIe, the caller only synchronises the stream -- no D2H copy launch, no allocation per call."""
        n = int(np.prod(shape))
        if getattr(self, "_host_out", None) is None or self._host_out.numel() < n:
            self._host_out = torch.empty(max(n, 1024), dtype=torch.float32).pin_memory()
        return self._host_out[:n].view(tuple(shape))

    def cem_plan(self, obs, cp_obs, cp_act, init_mean, init_var, n, seed=0, call=0, out=None):
        """`out`: optional [m,H,A] float32 destination (device tensor, or a pinned host tensor such as `host_out`)."""
        obs, init_mean, init_var = self._t(obs), self._t(init_mean), self._t(init_var)
        cp_obs = None if cp_obs is None else self._t(cp_obs)
        cp_act = None if cp_act is None else self._t(cp_act)
        m = obs.shape[0]
        self.ensure_rollout(None, m, max(1, n // self.dist_world))
        ws = self._workspace(m, n)
        if out is None:
            out = torch.empty((m, self.H, self.A), dtype=torch.float32, device=self.device)
        self._check(self.lib.cadm_cem_plan(self._ctx, ptr(obs), ptr(cp_obs), ptr(cp_act), ptr(init_mean), ptr(init_var), m, n,
                                     seed, call, ptr(ws), ptr(out), self.stream), "cadm_cem_plan")
        return out

    def cem_plan_host(self, arrays, n, seed=0, call=0, shapes=None):
        """The class API's fast path: `arrays` = (obs, cp_obs, cp_act, init_mean, init_var) as host arrays (None = absent) ->
        the plan [m,H,A] as a fresh numpy array.  Everything between is ONE library call (`cadm_cem_plan_staged`): the inputs
        go through a persistent pinned block, the plan comes back through another; the block layout is cached per shape set."""
        if shapes is None:
            shapes = tuple(None if a is None else tuple(np.shape(a)) for a in arrays)
        st = self._host_plan
        if st is None or st["shapes"] != shapes or st["n"] != n:
            offs, views, pos = [], [], 0
            sizes = [0 if sh is None else int(np.prod(sh)) for sh in shapes]
            total = max(sum(sizes), 1)
            host = torch.empty(total, dtype=torch.float32).pin_memory()
            hv = host.numpy()
            for sh, sz in zip(shapes, sizes):
                offs.append(-1 if sh is None else pos)
                views.append(None if sh is None else hv[pos:pos + sz].reshape(sh))
                pos += sz
            m = shapes[0][0]
            out = torch.zeros(m * self.H * self.A + 2 * m, dtype=torch.float32).pin_memory()   # plan + m completion flags + m mismatch words
            flags = out.numpy()[m * self.H * self.A + m:].view(np.uint32)
            st = self._host_plan = dict(shapes=shapes, n=n, ws=ptr(self._workspace(m, n)), host=host, views=views, dev=torch.empty(total, dtype=torch.float32, device=self.device),
                                        off=(ct.c_int32 * 5)(*offs), total=total, out=out, out_np=out.numpy()[:m * self.H * self.A].reshape(m, self.H, self.A), m=m, mismatch=flags,
                                        hp=ct.c_void_p(host.data_ptr()), op=ct.c_void_p(out.data_ptr()))
            st["dp"] = ct.c_void_p(st["dev"].data_ptr())
            self.ensure_rollout(None, m, max(1, n // self.dist_world))
        for v, a in zip(st["views"], arrays):
            if v is not None:
                np.copyto(v, a, casting="unsafe")
        rc = self.lib.cadm_cem_plan_staged(self._ctx, st["hp"], st["dp"], st["off"], st["total"], st["m"], n, seed, call,
                                           st["ws"], st["op"], 1, self.stream)
        if rc:
            self._check(rc, "cadm_cem_plan_staged")
        out = st["out_np"].copy()
        if self.dist_world > 1 and st["mismatch"].any():
            # the sharded refit compares the checksums every rank's all-gather payload carries (csrc/cem.hip: RefitRegen) and raises a
            # flag of its own: a NaN plan alone is also what a single-rank call returns for a non-finite observation
            self._check(self.lib.cadm_dist_mismatch(self._ctx, ct.byref(ct.c_int(0)), self.stream), "cadm_dist_mismatch")      # (resets the device word)
            raise RuntimeError(self.MISMATCH_MSG)
        return out

    MISMATCH_MSG = ("candidate-sharded planning: the ranks of the group were fed different obs / history / warm start on this call "
                    "(input checksums differ; the plan is NaN on every rank, and every rank raises on the same call)")

    def dist_mismatch(self):
        """Did the last sharded cem_plan see different replicated inputs on some rank?  Synchronises the stream; reading resets the flag."""
        v = ct.c_int(0)
        self._check(self.lib.cadm_dist_mismatch(self._ctx, ct.byref(v), self.stream), "cadm_dist_mismatch")
        return bool(v.value)

    def rs_plan(self, obs, cp_obs, cp_act, n, seed=0, call=0):
        obs = self._t(obs)
        cp_obs = None if cp_obs is None else self._t(cp_obs)
        cp_act = None if cp_act is None else self._t(cp_act)
        m = obs.shape[0]
        self.ensure_rollout(None, m, max(1, n // self.dist_world))
        ws = self._workspace(m, n)
        out = torch.empty((m, self.A), dtype=torch.float32, device=self.device)
        raw = torch.empty((m,), dtype=torch.int32, device=self.device) if self.discrete else None
        self._check(self.lib.cadm_rs_plan(self._ctx, ptr(obs), ptr(cp_obs), ptr(cp_act), m, n, seed, call, ptr(ws), ptr(out),
                                    ptr(raw), self.stream), "cadm_rs_plan")
        return raw if self.discrete else out

    # ------------------------------------------------------------------ iCEM planner (opt-in; csrc/icem.hip)
    def sample_actions_colored(self, mean, var, n, beta, xi=None, seed=0, call=0, it=0):
        """Candidates [m,n,H,A] with temporally correlated noise (`cadm_sample_actions_colored`).  xi [m,n,A,H]: injected spectral
        draws (slot 0 = x_0, then (x_k, y_k) in k order), or None to draw them on the device."""
        mean, var = self._t(mean), self._t(var)
        m = mean.shape[0]
        xi = None if xi is None else self._t(xi)
        if xi is not None and tuple(xi.shape) != (m, n, self.A, self.H):
            raise ValueError("sample_actions_colored: xi has shape %r, expected %r" % (tuple(xi.shape), (m, n, self.A, self.H)))
        out = torch.empty((m, n, self.H, self.A), dtype=torch.float32, device=self.device)
        self._check(self.lib.cadm_sample_actions_colored(self._ctx, ptr(mean), ptr(var), ptr(xi), float(beta), seed, call, it, m, n,
                                                         ptr(out), self.stream), "cadm_sample_actions_colored")
        return out

    def icem_keep(self, actions, elites, K):
        """actions [m,n,H,A], elites [m,num_elites] int32 (the refit's) -> the first K elites' sequences [m,K,H,A]."""
        m, n = actions.shape[0], actions.shape[1]
        out = torch.empty((m, K, self.H, self.A), dtype=torch.float32, device=self.device)
        self._check(self.lib.cadm_icem_keep(self._ctx, ptr(actions), ptr(elites), m, n, int(K), ptr(out), self.stream), "cadm_icem_keep")
        return out

    def icem_inject(self, actions, kept, valid=None, shift=0, slot0=0):
        """Write kept [m,K,H,A] into candidate slots [slot0, slot0 + K) of actions [m,n,H,A] IN PLACE (shift = 1: one step on,
        step H - 1 untouched; valid [m] int32: only envs with a non-zero flag)."""
        m, n, K = actions.shape[0], actions.shape[1], kept.shape[1]
        if not actions.is_contiguous() or not kept.is_contiguous() or slot0 < 0 or slot0 + K > n or kept.shape[0] != m:
            raise ValueError("icem_inject: slots [%d, %d) of %d candidates, kept %r" % (slot0, slot0 + K, n, tuple(kept.shape)))
        dst = ct.c_void_p(actions.data_ptr() + 4 * slot0 * self.H * self.A)
        self._check(self.lib.cadm_icem_inject(self._ctx, ptr(kept), ptr(valid), m, n, K, int(shift), dst, self.stream), "cadm_icem_inject")
        return actions

    def icem_track_best(self, cand, elites, actions, best_ret, best_seq):
        """best_ret [m] / best_seq [m,H,A] updated IN PLACE where this iteration's best candidate -- the greatest non-NaN return: the
        first elite whose return is not NaN, the arg-max over cand when all are NaN -- is strictly better, or best_ret is NaN."""
        m, n = actions.shape[0], actions.shape[1]
        self._check(self.lib.cadm_icem_track_best(self._ctx, ptr(cand), ptr(elites), ptr(actions), m, n, ptr(best_ret), ptr(best_seq),
                                                  self.stream), "cadm_icem_track_best")

    @staticmethod
    def icem_params(noise_beta=0.0, keep_elites=0, decay=1.0, return_best=False, add_mean_last=False):
        prm = _lib.IcemParams()
        prm.noise_beta, prm.keep_elites, prm.decay = float(noise_beta), int(keep_elites), float(decay)
        prm.return_best, prm.add_mean_last = int(bool(return_best)), int(bool(add_mean_last))
        return prm

    def icem_candidates(self, n, decay, it, keep_elites=0):
        """Candidates of CEM iteration `it`: min(n, max(floor(n / decay^it), 2 num_elites, K + 1)), decay rounded to float32 as the
        library receives it (csrc/icem.hip icem_n_it)."""
        v = int(np.floor(float(n) / float(np.float32(decay)) ** it))
        return min(n, max(v, 2 * self.num_elites, keep_elites + 1))

    def icem_plan(self, params, obs, cp_obs, cp_act, init_mean, init_var, n, carry=None, carry_valid=None, seed=0, call=0, out=None,
                  want_best_return=False):
        """`cadm_icem_plan`.  carry [m,K,H,A] float32 / carry_valid [m] int32: caller-owned device tensors, read at iteration 0 and
        rewritten after the last refit (required when params.keep_elites > 0).  `out` as in `cem_plan`."""
        return self._loop_plan("icem_plan", self.lib.cadm_icem_plan, (ct.byref(params),), False, params.keep_elites, obs, cp_obs, cp_act,
                               init_mean, init_var, n, carry, carry_valid, seed, call, out, want_best_return)

    def _loop_plan(self, who, export, head, mppi, K, obs, cp_obs, cp_act, init_mean, init_var, n, carry, carry_valid, seed, call, out,
                   want_best_return, traj=False, track=None, act=False, unc=None, val=None, rew=None, pol=None, crt=None, anc=None):
        """What `icem_plan`, `mppi_plan` and `scored_plan` share: staging, the carry check, the workspace, the outputs and the call of
        `export` (cadm_<who>) -- head: its arguments between the ctx and obs; mppi: which update's workspace; K: keep_elites; traj: the
        workspace with the trajectory view behind it (a constrained loop); track: as in `_loop_workspace` (a tracked loop); act: the workspace of an actuated loop;
        unc: None, or the (terminate, actuator) of a loop with an uncertainty term, whose slot it is; val: None, or the (terminate, actuator,
        uncertainty) of a loop with a terminal value, whose slot it is; rew: likewise for a loop with a learned reward; pol: None, or the
        (terminate, actuator, uncertainty, P) of a loop with a policy prior, whose slot it is; crt: likewise for a loop with a terminal Q;
        anc: likewise for a loop with the actor's log-density."""
        obs, init_mean, init_var = self._t(obs), self._t(init_mean), self._t(init_var)
        cp_obs = None if cp_obs is None else self._t(cp_obs)
        cp_act = None if cp_act is None else self._t(cp_act)
        m, K = obs.shape[0], int(K)
        if K > 0 and (carry is None or carry_valid is None or tuple(carry.shape) != (m, K, self.H, self.A) or carry.dtype != torch.float32
                      or tuple(carry_valid.shape) != (m,) or carry_valid.dtype != torch.int32 or not carry.is_contiguous()):
            raise ValueError("%s: keep_elites=%d needs carry [%d,%d,%d,%d] float32 and carry_valid [%d] int32" % (who, K, m, K, self.H, self.A, m))
        self.ensure_rollout(None, m, n)
        ws = self._loop_workspace(mppi, m, n, K, traj=traj, track=track, act=act, unc=unc, val=val, rew=rew, pol=pol, crt=crt, anc=anc)
        if out is None:
            out = torch.empty((m, self.H, self.A), dtype=torch.float32, device=self.device)
        best = torch.empty((m,), dtype=torch.float32, device=self.device) if want_best_return else None
        self._check(export(self._ctx, *head, ptr(obs), ptr(cp_obs), ptr(cp_act), ptr(init_mean), ptr(init_var), ptr(carry), ptr(carry_valid),
                           m, n, seed, call, ptr(ws), ptr(out), ptr(best), self.stream), "cadm_" + who)
        return (out, best) if want_best_return else out

    def opt_in_plan(self, opt, *args, phase=None, targets=None, target_offset=None, act_prev=None, act_prefix=None, **kw):
        """The opt-in loop under a `planner.PlanOptions`: `actuated_plan` when it holds an actuator model (act_prev [m,A] / act_prefix
        [m,delay,A]: the envs' actuator state, moved on in place when the options say so), `tracking_plan` when it holds tracking terms (targets [m,T,K] or [m,K],
        target_offset [m] int32 or None = 0), `knot_plan` when it holds knots (phase: the envs' grid phases [m] int32, None = 0),
        `constrained_plan` when it holds constraints, `scored_plan` when it holds a score, else `mppi_plan` or `icem_plan` by its update.
        Arguments as `icem_plan` behind its params.  First of all `rewarded_plan`, when it holds a learned reward, then `valued_plan`, when
        it holds a terminal value, then `uncertain_plan`, when it holds an uncertainty term.  Before all of them `guided_plan`, when it
        holds a policy prior; and before that `critic_plan`, when it holds a terminal Q; outermost `anchored_plan`, when it holds the
        actor's log-density."""
        full = (getattr(opt, "logp_params", None), getattr(opt, "critic_params", None), getattr(opt, "policy_params", None), getattr(opt, "reward_params", None),
                getattr(opt, "value_params", None), getattr(opt, "uncertainty_params", None), opt.actuator_params, act_prev, act_prefix,
                getattr(opt, "action_advance", None), opt.track_params, targets, target_offset, opt.knot_params, phase,
                opt.constraint_params, opt.score_params, opt.params)      # the outermost method's arguments
        for method, own in _PLAN_ROUTES:      # the outermost level whose own struct the options hold
            if full[own] is not None:
                return getattr(self, method)(*full[own:], *args, **kw)
        return (self.mppi_plan if opt.update == "mppi" else self.icem_plan)(opt.params, *args, **kw)

    def _nest_plan(self, level, lead, obs, cp_obs, cp_act, init_mean, init_var, n, carry, carry_valid, seed, call, out, want_best_return):
        """What the eleven nested `*_plan` methods do (`_PLAN_NEST`); level: the method called, lead: its arguments in front of obs.  Finds
        the level that answers -- its name is the one in the messages, its export the one called, its slot the workspace --, checks what
        the host can check, builds the export's arguments between the ctx and obs, and calls `_loop_plan`."""
        i = _PLAN_LEVEL[level]
        full = (None,) * (_PLAN_NARGS[-1] - len(lead)) + lead
        while i >= _ACTUATED and full[-_PLAN_NARGS[i]] is None:
            i -= 1
        who, _, tag, nflags = _PLAN_NEST[i]
        (logp, critic, policy, reward, value, uncertainty, actuator, prev, prefix, advance, track, targets, offset, knots, phase, constraints,
         score, params) = full
        mppi, params = self._as_mppi_params(params)
        m = int(np.shape(obs)[0]) if i >= _KNOT else None      # (the two levels below have nothing per env to check)
        if actuator is None:
            prev = prefix = None
        else:
            for name, t in (("prev", prev), ("prefix", prefix)):
                if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32):
                    raise ValueError("%s: %s must be a float32 device tensor (it is moved on in place)" % (who, name))
            if prev is None or (prefix is None and actuator.delay > 0):
                raise ValueError("%s: the actuator model needs prev [m,A], and prefix [m,delay,A] with a delay" % who)
            prev, prefix = self._actuator_state(prev, prefix, m, actuator.delay, who)
        phase = self._phase(phase, m, who)
        T = 0
        if track is None:      # the library's own route to the loop underneath, with that loop's workspace
            targets = offset = None
        else:
            targets, T, offset = self._targets(targets, offset, m, track.n, who)
        head = (_by(logp), _by(critic), _by(policy), _by(reward), _by(value), _by(uncertainty), _by(actuator), ptr(prev), ptr(prefix), int(bool(advance)),
                _by(track), ptr(targets), T, ptr(offset), _by(knots), ptr(phase), _by(constraints), _by(score), int(mppi), ct.byref(params))
        terminate = constraints is not None and constraints.mode == _lib.CONSTRAIN_MODES["terminate"]
        flags = (terminate, actuator is not None, uncertainty is not None, 0 if policy is None else max(int(policy.n_samples), 0))
        ws = {tag: flags[:nflags]} if tag else dict(traj=constraints is not None, track=None if track is None else terminate,
                                                    act=actuator is not None)
        return self._loop_plan(who, getattr(self.lib, "cadm_" + who), head[-_PLAN_NHEAD[i]:], mppi, params.icem.keep_elites, obs, cp_obs,
                               cp_act, init_mean, init_var, n, carry, carry_valid, seed, call, out, want_best_return, **ws)

    def _loop_workspace(self, mppi, m, n, K, traj=False, track=None, act=False, unc=None, val=None, rew=None, pol=None, crt=None, anc=None):
        """The opt-in loop's workspace, cached per (m, n, K): one for the elite refit, a larger one for the MPPI update, and -- only for a
        constrained loop -- each of them with the trajectory view behind it (an unconstrained model never allocates that).  track: None,
        or whether a tracked loop runs under TERMINATE constraints -- the tracking slot (`cadm_tracking_workspace_bytes`: the trajectory
        view, and the first-violation view in front of it under TERMINATE).  act: an actuated loop's slot (`cadm_actuated_workspace_bytes`:
        the loop underneath's views, and behind them the candidates' rate cost and the plan's device copy).  unc: None, or (terminate,
        actuator) -- the slot of a loop with an uncertainty term (`cadm_uncertain_workspace_bytes`: always with the trajectory view, the
        first-violation view under TERMINATE constraints, the actuator's views, and behind everything the step costs and the cost).  val:
        None, or (terminate, actuator, uncertainty) -- the slot of a loop with a terminal value (`cadm_valued_workspace_bytes`).  rew:
        None, or (terminate, actuator, uncertainty) -- the slot of a loop with a learned reward (`cadm_rewarded_workspace_bytes`: the
        valued loop's, and behind everything the step rewards).  pol: None, or (terminate, actuator, uncertainty, P) -- the slot of a loop
        with a policy prior (`cadm_guided_workspace_bytes`: the rewarded loop's, and behind everything the proposals and the roll's
        workspace).  crt: None, or (terminate, actuator, uncertainty, P) -- the slot of a loop with a terminal Q
        (`cadm_critic_workspace_bytes`: the guided loop's; P = 0 without a policy prior in the same call).  anc: likewise -- the slot of
        a loop with the actor's log-density (`cadm_anchored_workspace_bytes`: the critic loop's, and behind everything the step
        log-densities)."""
        mppi = bool(mppi)
        for (tag, size), flags in zip(_PLAN_SLOTS, (anc, crt, pol, rew, val, unc)):      # the outermost term given names the slot and sizes it
            if flags is not None:
                flags = tuple(bool(f) for f in flags[:3]) + tuple(int(P) for P in flags[3:])
                slot = (mppi, tag) + flags
                break
        else:                                                  # the levels below: a slot per combination of what they are given
            slot = (mppi, bool(traj)) if track is None else (mppi, "track", bool(track))
            if act:
                slot, size, flags = slot + ("act",), "cadm_actuated_workspace_bytes", (bool(traj) or track is not None, bool(track))
            elif track is not None:
                size, flags = "cadm_tracking_workspace_bytes", (bool(track),)
            elif traj:
                size, flags = "cadm_constrained_workspace_bytes", ()
            else:                                              # (the two plain ones take no update flag: one export each)
                size, flags = "cadm_mppi_workspace_bytes" if mppi else "cadm_icem_workspace_bytes", None
        key, ws = self._loop_ws.get(slot, (None, None))
        if key != (m, n, K):
            nbytes = getattr(self.lib, size)(self._ctx, m, n, K, *(() if flags is None else (int(mppi),) + tuple(int(f) for f in flags)))
            ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=self.device)
            self._loop_ws[slot] = ((m, n, K), ws)
        return ws

    # ------------------------------------------------------------------ MPPI update (opt-in; csrc/mppi.hip)
    def mppi_refit(self, cand, actions, mean, var, temperature=1.0, relative=False, want_plan=False):
        """`cadm_mppi_refit`: cand [m,n], actions [m,n,H,A]; mean / var [m,H,A] updated IN PLACE with the softmax-weighted statistics of
        ALL candidates (weights exp((R - max R) / lambda); `relative`: lambda is a fraction of the env's return range).  want_plan:
        also returns clip(new mean) [m,H,A]."""
        m, n = actions.shape[0], actions.shape[1]
        if tuple(cand.shape) != (m, n) or tuple(mean.shape) != (m, self.H, self.A) or tuple(var.shape) != (m, self.H, self.A):
            raise ValueError("mppi_refit: cand %r, actions %r, mean %r, var %r do not agree" % (tuple(cand.shape), tuple(actions.shape),
                                                                                           tuple(mean.shape), tuple(var.shape)))
        plan = torch.empty((m, self.H, self.A), dtype=torch.float32, device=self.device) if want_plan else None
        self._check(self.lib.cadm_mppi_refit(self._ctx, ptr(cand), ptr(actions), m, n, float(temperature), int(bool(relative)), ptr(mean),
                                             ptr(var), ptr(plan), self.stream), "cadm_mppi_refit")
        return plan

    @staticmethod
    def mppi_params(temperature=1.0, relative=False, **icem):
        """`cadm_mppi_params`: the switches of `icem_params` plus the temperature and its relative flag."""
        prm = _lib.MppiParams()
        prm.icem = HipEngine.icem_params(**icem)
        prm.temperature, prm.relative = float(temperature), int(bool(relative))
        return prm

    def mppi_plan(self, params, obs, cp_obs, cp_act, init_mean, init_var, n, carry=None, carry_valid=None, seed=0, call=0, out=None,
                  want_best_return=False):
        """`cadm_mppi_plan`: the loop of `icem_plan` with the MPPI update in place of the elite refit.  Arguments as `icem_plan`."""
        return self._loop_plan("mppi_plan", self.lib.cadm_mppi_plan, (ct.byref(params),), True, params.icem.keep_elites, obs, cp_obs, cp_act,
                               init_mean, init_var, n, carry, carry_valid, seed, call, out, want_best_return)

    # ------------------------------------------------------------------ risk-aware candidate scores (opt-in; csrc/score.hip)
    @staticmethod
    def score_params(mode="mean", kappa=0.0, k=None):
        """`cadm_score_params`.  mode: "mean" | "mean_std" | "member_std" | "cvar" (or its CADM_SCORE_* number); kappa: the weight of the
        standard deviation (the std modes); k: how many of the lowest particle returns are averaged (cvar)."""
        prm = _lib.ScoreParams()
        prm.mode = _lib.SCORE_MODES[mode] if isinstance(mode, str) else int(mode)
        prm.kappa, prm.k = float(kappa), 0 if k is None else int(k)
        return prm

    @staticmethod
    def cvar_k(alpha, p):
        """The tail fraction alpha in (0, 1] of p particles as a count: min(p, max(1, ceil(alpha p))), alpha p rounded to 6 decimals first
        (0.1 * 20 is 2.0000000000000004 in binary: 2 particles, not 3)."""
        return int(min(p, max(1, math.ceil(round(float(alpha) * p, 6)))))

    def particle_score(self, rows, mode, kappa=0.0, k=None):
        """`cadm_particle_score`: rows [m,n_local,p] -> the candidates' scores [m,n_local] (mode "mean": `particle_mean`'s bits).
        mode: a name or number as in `score_params`, or a `score_params` result."""
        rows = self._t(rows)
        if rows.dim() != 3 or rows.shape[2] != self.p or not rows.is_contiguous():
            raise ValueError("particle_score: rows %r, expected [m, n_local, %d] contiguous" % (tuple(rows.shape), self.p))
        m, n_local = rows.shape[0], rows.shape[1]
        prm = mode if isinstance(mode, _lib.ScoreParams) else self.score_params(mode, kappa, k)
        out = torch.empty((m, n_local), dtype=torch.float32, device=self.device)
        self._check(self.lib.cadm_particle_score(self._ctx, ptr(rows), m, n_local, ct.byref(prm), ptr(out), self.stream), "cadm_particle_score")
        return out

    @staticmethod
    def _as_mppi_params(params):
        """(is it an MPPI loop, the `cadm_mppi_params` the scored / constrained / knot exports take): an `icem_params` result is wrapped."""
        if isinstance(params, _lib.MppiParams):
            return True, params
        full = _lib.MppiParams()
        full.icem, full.temperature = params, 1.0
        return False, full

    def scored_plan(self, score, params, obs, cp_obs, cp_act, init_mean, init_var, n, carry=None, carry_valid=None, seed=0, call=0, out=None,
                    want_best_return=False):
        """`cadm_scored_plan`: the loop of `icem_plan` (params from `icem_params`) or of `mppi_plan` (params from `mppi_params`) with
        `score` (`score_params`; None = the mean) in place of the particle mean.  The best return is then the best score.  Arguments as
        `icem_plan`; the workspaces are the ones those two cache."""
        return self._nest_plan("scored_plan", (score, params), obs, cp_obs, cp_act, init_mean, init_var, n, carry, carry_valid, seed, call,
                               out, want_best_return)

    # ------------------------------------------------------------------ state constraints and termination (opt-in; csrc/constrain.hip)
    @staticmethod
    def constraint_params(constraints, mode="penalty", weight=None):
        """`cadm_constraint_params` from a list of dict(dim=d, lo=..., hi=...): a state is healthy iff lo < x[d] < hi for every entry (a
        missing side: -inf / +inf; at least one is given, and lo < hi).  mode: "penalty" | "terminate" (or its CADM_CONSTRAIN_* number);
        weight: finite, >= 0 -- per violating step (penalty), or once at the first one (terminate).  Everything that needs no engine is
        checked here; a dim beyond the engine's D is refused by the library."""
        if isinstance(constraints, dict):
            constraints = [constraints]
        try:
            cons = list(constraints)
        except TypeError:
            raise ValueError("constraints must be a list of dict(dim=, lo=, hi=), got %r" % (constraints,)) from None
        if not 1 <= len(cons) <= _lib.MAX_CONSTRAINTS:
            raise ValueError("constraints: %d entries, expected 1 .. %d" % (len(cons), _lib.MAX_CONSTRAINTS))
        if isinstance(mode, str):
            if mode not in _lib.CONSTRAIN_MODES:
                raise ValueError("constraint mode must be 'penalty' or 'terminate', got %r" % (mode,))
            mode = _lib.CONSTRAIN_MODES[mode]
        elif int(mode) not in _lib.CONSTRAIN_MODES.values():
            raise ValueError("constraint mode must be 'penalty' or 'terminate', got %r" % (mode,))
        if weight is None or not math.isfinite(float(weight)) or float(weight) < 0.0:
            raise ValueError("constraints need a weight that is finite and >= 0, got %r" % (weight,))
        prm = _lib.ConstraintParams()
        prm.n, prm.mode, prm.weight = len(cons), int(mode), float(weight)
        for k, c in enumerate(cons):
            if not isinstance(c, dict) or "dim" not in c or set(c) - {"dim", "lo", "hi"}:
                raise ValueError("constraint %d: expected dict(dim=, lo=, hi=), got %r" % (k, c))
            lo, hi = c.get("lo"), c.get("hi")
            if lo is None and hi is None:
                raise ValueError("constraint %d: at least one of lo and hi is needed" % k)
            if isinstance(c["dim"], bool) or not isinstance(c["dim"], (int, np.integer)) or int(c["dim"]) < 0:
                raise ValueError("constraint %d: dim must be an observation index >= 0, got %r" % (k, c["dim"]))
            lo = -math.inf if lo is None else float(np.float32(lo))      # (the bounds as the kernel compares them)
            hi = math.inf if hi is None else float(np.float32(hi))
            if math.isnan(lo) or math.isnan(hi):
                raise ValueError("constraint %d: a bound is NaN" % k)
            if not lo < hi:
                raise ValueError("constraint %d: lo %r must be below hi %r (in float32)" % (k, lo, hi))
            if math.isinf(lo) and math.isinf(hi):
                raise ValueError("constraint %d: both sides are infinite: it constrains nothing" % k)
            prm.dim[k], prm.lo[k], prm.hi[k] = int(c["dim"]), lo, hi
        return prm

    def constrain_returns(self, traj, rows, constraints, mode="penalty", weight=None, obs=None, actions=None, out=None):
        """`cadm_constrain_returns` on device tensors: traj [H,m,n,p,D] (a rollout's `traj_out`), rows [m,n,p] (its returns) ->
        (rows' [m,n,p], first_violation [m,n,p] int32, violations [m,n,p] int32).  constraints: a `constraint_params` result, or the
        list it takes (then with mode and weight).  obs [m,D] / actions [m,n,H,A] raw: needed in terminate mode.  out: where rows' go
        (may be `rows` itself)."""
        prm = constraints if isinstance(constraints, _lib.ConstraintParams) else self.constraint_params(constraints, mode, weight)
        traj, rows = self._t(traj), self._t(rows)
        obs = None if obs is None else self._t(obs)
        actions = None if actions is None else self._t(actions)
        if traj.dim() != 5 or rows.dim() != 3:
            raise ValueError("constrain_returns: traj %r, rows %r: expected contiguous [H,m,n,p,D] and [m,n,p]" % (tuple(traj.shape), tuple(rows.shape)))
        H, m, n, p, D = traj.shape
        if (H, p, D) != (self.H, self.p, self.D) or tuple(rows.shape) != (m, n, p):
            raise ValueError("constrain_returns: traj %r, rows %r do not agree with the engine (H=%d, p=%d, D=%d)"
                             % (tuple(traj.shape), tuple(rows.shape), self.H, self.p, self.D))
        if obs is not None and tuple(obs.shape) != (m, D) or actions is not None and tuple(actions.shape) != (m, n, H, self.A):
            raise ValueError("constrain_returns: obs %r, actions %r: expected [%d,%d] and [%d,%d,%d,%d]"
                             % (None if obs is None else tuple(obs.shape), None if actions is None else tuple(actions.shape), m, D, m, n, H, self.A))
        if out is None:
            out = torch.empty_like(rows)
        elif tuple(out.shape) != (m, n, p) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("constrain_returns: out %r, expected contiguous float32 %r" % (tuple(out.shape), (m, n, p)))
        first = torch.empty((m, n, p), dtype=torch.int32, device=self.device)
        viol = torch.empty((m, n, p), dtype=torch.int32, device=self.device)
        self._check(self.lib.cadm_constrain_returns(self._ctx, ct.byref(prm), ptr(traj), ptr(obs), ptr(actions), ptr(rows), m, n, ptr(out),
                                                    ptr(first), ptr(viol), self.stream), "cadm_constrain_returns")
        return out, first, viol

    def constrained_plan(self, constraints, score, params, obs, cp_obs, cp_act, init_mean, init_var, n, carry=None, carry_valid=None, seed=0,
                         call=0, out=None, want_best_return=False):
        """`cadm_constrained_plan`: the loop of `scored_plan` with `constraints` (`constraint_params`; None = none, and `scored_plan`'s
        launches) rewriting every iteration's particle returns before the score.  Arguments behind `constraints` as `scored_plan`; with
        constraints the workspace carries the trajectory view (`cadm_constrained_workspace_bytes`), cached apart from the plain ones."""
        return self._nest_plan("constrained_plan", (constraints, score, params), obs, cp_obs, cp_act, init_mean, init_var, n, carry,
                               carry_valid, seed, call, out, want_best_return)

    # ------------------------------------------------------------------ discount over the horizon (opt-in; csrc/discount.hip)
    def set_discount(self, gamma):
        """`cadm_set_discount`: gamma in (0, 1]; 1.0 clears the discount.  State of the engine, as the horizon is: from here on the opt-in
        loop and every stand-alone stage call weigh step t by gamma^t (`discount_weights`), and `cem_plan` / `rs_plan` refuse.  The
        loop records trajectories under a discount, so every cached loop workspace is dropped and sized again at the next plan."""
        gamma = float(gamma)
        if not (0.0 < gamma <= 1.0):      # (NaN: false)
            raise ValueError("set_discount: the discount %r is not in (0, 1]" % (gamma,))
        with torch.cuda.device(self.device):
            self._check(self.lib.cadm_set_discount(self._ctx, gamma, self.stream), "cadm_set_discount")
        self._loop_ws = {}

    def discount_weights(self):
        """`cadm_discount_weights`: the floats the kernels read, float32 [H + 1] (gamma^t, t = 0 .. H), or None while no discount is set."""
        out = np.empty((self.H + 1,), np.float32)
        is_set = ct.c_int(0)
        self._check(self.lib.cadm_discount_weights(self._ctx, out.ctypes.data_as(ct.POINTER(ct.c_float)), ct.byref(is_set)),
                    "cadm_discount_weights")
        return out if is_set.value else None

    def discount_returns(self, traj, obs, actions, rows, want_steps=False, out=None):
        """`cadm_discount_returns` on device tensors: traj [H,m,n,p,D] (a rollout's `traj_out`), obs [m,D], actions [m,n,H,A] raw, rows
        [m,n,p] (its returns: a NaN stays) -> the discounted env returns [m,n,p]; want_steps: also the undiscounted step rewards
        [H,m,n,p].  out: where the returns go (may be `rows` itself).  Needs a discount (`set_discount`)."""
        traj, obs, actions, rows = self._t(traj), self._t(obs), self._t(actions), self._t(rows)
        if traj.dim() != 5 or rows.dim() != 3:
            raise ValueError("discount_returns: traj %r, rows %r: expected [H,m,n,p,D] and [m,n,p]" % (tuple(traj.shape), tuple(rows.shape)))
        H, m, n, p, D = traj.shape
        if (H, p, D) != (self.H, self.p, self.D) or tuple(rows.shape) != (m, n, p):
            raise ValueError("discount_returns: traj %r, rows %r do not agree with the engine (H=%d, p=%d, D=%d)"
                             % (tuple(traj.shape), tuple(rows.shape), self.H, self.p, self.D))
        if tuple(obs.shape) != (m, D) or tuple(actions.shape) != (m, n, H, self.A):
            raise ValueError("discount_returns: obs %r, actions %r: expected [%d,%d] and [%d,%d,%d,%d]"
                             % (tuple(obs.shape), tuple(actions.shape), m, D, m, n, H, self.A))
        if out is None:
            out = torch.empty_like(rows)
        elif tuple(out.shape) != (m, n, p) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("discount_returns: out %r, expected contiguous float32 %r" % (tuple(out.shape), (m, n, p)))
        steps = torch.empty((H, m, n, p), dtype=torch.float32, device=self.device) if want_steps else None
        self._check(self.lib.cadm_discount_returns(self._ctx, ptr(traj), ptr(obs), ptr(actions), m, n, ptr(rows), ptr(out), ptr(steps),
                                                   self.stream), "cadm_discount_returns")
        return (out, steps) if want_steps else out

    # ------------------------------------------------------------------ plans on knots (opt-in; csrc/knots.hip)
    @staticmethod
    def knot_params(spacing, interp="hold"):
        """`cadm_knot_params`: knot steps `spacing` >= 1 apart (1: every step is a knot); interp: "hold" | "linear" (or its CADM_KNOT_*
        number) -- action repeat, or linear interpolation between knots."""
        if isinstance(spacing, bool) or not isinstance(spacing, (int, np.integer)) or int(spacing) < 1:
            raise ValueError("knot spacing must be an integer >= 1, got %r" % (spacing,))
        if isinstance(interp, str):
            if interp not in _lib.KNOT_INTERPS:
                raise ValueError("knot interp must be 'hold' or 'linear', got %r" % (interp,))
            interp = _lib.KNOT_INTERPS[interp]
        elif int(interp) not in _lib.KNOT_INTERPS.values():
            raise ValueError("knot interp must be 'hold' or 'linear', got %r" % (interp,))
        prm = _lib.KnotParams()
        prm.spacing, prm.interp = int(spacing), int(interp)
        return prm

    def _phase(self, phase, m, who):
        """phase [m] int32 on the device (None stays None: phase 0 for every env)"""
        if phase is None:
            return None
        phase = self._t(phase, dtype=torch.int32)
        if tuple(phase.shape) != (m,) or not phase.is_contiguous():
            raise ValueError("%s: phase %r, expected [%d] int32" % (who, tuple(phase.shape), m))
        return phase

    def shape_actions(self, seqs, knots, phase=None):
        """`cadm_shape_actions`: seqs [m,n,H,A] or [m,H,A] (a contiguous float32 device tensor) shaped onto the grid of `knots`
        (`knot_params`) IN PLACE; phase [m] int32 (None: 0 for every env).  Returns seqs."""
        if not isinstance(seqs, torch.Tensor) or seqs.dtype != torch.float32 or not seqs.is_contiguous() or seqs.dim() not in (3, 4) \
                or tuple(seqs.shape[-2:]) != (self.H, self.A) or seqs.shape[0] == 0 or not seqs.is_cuda:
            raise ValueError("shape_actions: expected a contiguous float32 device tensor [m,n,%d,%d] or [m,%d,%d]" % (self.H, self.A, self.H, self.A))
        m, n = seqs.shape[0], seqs.shape[1] if seqs.dim() == 4 else 1
        phase = self._phase(phase, m, "shape_actions")
        self._check(self.lib.cadm_shape_actions(self._ctx, ct.byref(knots), ptr(phase), m, n, ptr(seqs), self.stream), "cadm_shape_actions")
        return seqs

    def knot_plan(self, knots, phase, constraints, score, params, obs, cp_obs, cp_act, init_mean, init_var, n, carry=None, carry_valid=None,
                  seed=0, call=0, out=None, want_best_return=False):
        """`cadm_knot_plan`: the loop of `constrained_plan` with every iteration's candidates shaped onto the grid of `knots`
        (`knot_params`; None = none, and `constrained_plan`'s launches) before the rollout; phase [m] int32 (None: 0 for every env).
        Arguments behind `phase` as `constrained_plan`, and its workspaces."""
        return self._nest_plan("knot_plan", (knots, phase, constraints, score, params), obs, cp_obs, cp_act, init_mean, init_var, n, carry,
                               carry_valid, seed, call, out, want_best_return)

    # ------------------------------------------------------------------ tracking targets at run time (opt-in; csrc/tracking.hip)
    @staticmethod
    def track_params(terms):
        """`cadm_track_params` from a list of dict(dim=d, kind="square" | "abs" | "huber", w=..., delta=...): term k costs w * c(x[d] - target k),
        c = e^2, |e|, or the Huber function with threshold delta (kind: a name or its CADM_TRACK_* number; default "square"; w: finite,
        >= 0, default 1; delta: finite, > 0, for "huber" only and required there).  Everything that needs no engine is checked here; a dim
        beyond the engine's D is refused by the library."""
        if isinstance(terms, dict):
            terms = [terms]
        try:
            terms = list(terms)
        except TypeError:
            raise ValueError("tracking terms must be a list of dict(dim=, kind=, w=, delta=), got %r" % (terms,)) from None
        if not 1 <= len(terms) <= _lib.MAX_TRACK_TERMS:
            raise ValueError("tracking: %d terms, expected 1 .. %d" % (len(terms), _lib.MAX_TRACK_TERMS))
        prm = _lib.TrackParams()
        prm.n = len(terms)
        for k, c in enumerate(terms):
            if not isinstance(c, dict) or "dim" not in c or set(c) - {"dim", "kind", "w", "delta"}:
                raise ValueError("tracking term %d: expected dict(dim=, kind=, w=, delta=), got %r" % (k, c))
            if isinstance(c["dim"], bool) or not isinstance(c["dim"], (int, np.integer)) or int(c["dim"]) < 0:
                raise ValueError("tracking term %d: dim must be an observation index >= 0, got %r" % (k, c["dim"]))
            kind = c.get("kind", "square")
            if isinstance(kind, str):
                if kind not in _lib.TRACK_KINDS:
                    raise ValueError("tracking term %d: kind must be 'square', 'abs' or 'huber', got %r" % (k, kind))
                kind = _lib.TRACK_KINDS[kind]
            elif isinstance(kind, bool) or not isinstance(kind, (int, np.integer)) or int(kind) not in _lib.TRACK_KINDS.values():
                raise ValueError("tracking term %d: kind must be 'square', 'abs' or 'huber', got %r" % (k, kind))
            w = float(np.float32(c.get("w", 1.0)))      # (the weight as the kernel multiplies by it)
            if not math.isfinite(w) or w < 0.0:
                raise ValueError("tracking term %d: w must be finite and >= 0, got %r" % (k, c.get("w")))
            delta = c.get("delta")
            if int(kind) == _lib.TRACK_KINDS["huber"]:
                if delta is None or not math.isfinite(float(np.float32(delta))) or float(np.float32(delta)) <= 0.0:
                    raise ValueError("tracking term %d: kind 'huber' needs a delta that is finite and > 0, got %r" % (k, delta))
            elif delta is not None:
                raise ValueError("tracking term %d: delta configures kind 'huber' only" % k)
            prm.dim[k], prm.kind[k], prm.w[k], prm.delta[k] = int(c["dim"]), int(kind), w, 0.0 if delta is None else float(np.float32(delta))
        return prm

    def _targets(self, targets, offset, m, K, who):
        """(targets [m,T,K] float32 contiguous on the device -- [m,K] is T = 1 --, T, offset [m] int32 on the device or None)"""
        if targets is None:
            raise ValueError("%s: tracking terms need targets" % who)
        targets = self._t(targets)
        if targets.dim() == 2:
            targets = targets[:, None]
        if targets.dim() != 3 or targets.shape[0] != m or targets.shape[1] < 1 or targets.shape[2] != K:
            raise ValueError("%s: targets %r, expected [%d,T,%d] with T >= 1 or [%d,%d]" % (who, tuple(targets.shape), m, K, m, K))
        targets = targets.contiguous()
        if offset is not None:
            offset = self._t(offset, dtype=torch.int32)
            if tuple(offset.shape) != (m,):
                raise ValueError("%s: offset %r, expected [%d] int32" % (who, tuple(offset.shape), m))
        return targets, int(targets.shape[1]), offset

    def tracking_returns(self, traj, rows, track, targets, offset=None, first=None, out=None, want_cost=False):
        """`cadm_tracking_returns` on device tensors: traj [H,m,n,p,D] (a rollout's `traj_out`), rows [m,n,p] (its returns, or what
        `constrain_returns` made of them) -> rows' [m,n,p] = rows - cost (with want_cost: (rows', cost [m,n,p])).  track: a `track_params`
        result, or the list it takes.  targets [m,T,K] or [m,K]; offset [m] int32 (None: 0); first [m,n,p] int32 (None: every step
        counts): `constrain_returns`' first_violation -- steps behind it are not counted.  out: where rows' go (may be `rows` itself)."""
        prm = track if isinstance(track, _lib.TrackParams) else self.track_params(track)
        traj, rows, first, out = HipEngine._returns_args(self, "tracking_returns", traj, rows, first, out)
        H, m, n, p, D = traj.shape
        targets, T, offset = self._targets(targets, offset, m, prm.n, "tracking_returns")
        cost = torch.empty((m, n, p), dtype=torch.float32, device=self.device) if want_cost else None
        self._check(self.lib.cadm_tracking_returns(self._ctx, ct.byref(prm), ptr(traj), ptr(targets), T, ptr(offset), ptr(first), ptr(rows), m, n,
                                                   ptr(out), ptr(cost), self.stream), "cadm_tracking_returns")
        return (out, cost) if want_cost else out

    def tracking_plan(self, track, targets, offset, knots, phase, constraints, score, params, obs, cp_obs, cp_act, init_mean, init_var, n,
                      carry=None, carry_valid=None, seed=0, call=0, out=None, want_best_return=False):
        """`cadm_tracking_plan`: the loop of `knot_plan` with the cost of `track` (`track_params`; None = none, and `knot_plan`'s launches)
        against targets [m,T,K] or [m,K] at offset [m] int32 (None: 0 for every env) taken off every iteration's particle returns, behind
        the constraints and before the score.  Arguments behind `offset` as `knot_plan`; with terms the workspace is the tracking slot
        (`cadm_tracking_workspace_bytes`), cached apart from the others."""
        return self._nest_plan("tracking_plan", (track, targets, offset, knots, phase, constraints, score, params), obs, cp_obs, cp_act,
                               init_mean, init_var, n, carry, carry_valid, seed, call, out, want_best_return)

    # ------------------------------------------------------------------ actuator model (opt-in; csrc/actuator.hip)
    @staticmethod
    def actuator_params(delay=0, rate_limit=None, rate_cost=None, action_dim=None, horizon=None):
        """`cadm_actuator_params`: delay -- an integer >= 0, the number of leading plan steps earlier calls have committed (below
        `horizon` when that is given); rate_limit -- None (none), a scalar or [A]: how far an action dim may move per step, > 0, inf = no
        limit for that dim; rate_cost -- None (0), a scalar or [A]: the weight of (u_t - u_{t-1})^2 per dim, finite and >= 0.  Arrays
        must have `action_dim` entries when that is given, at most `_lib.MAX_ACT_DIMS` anyway, and agree with one another; the library
        checks them, and the delay, against the engine's A and H.  Needs no GPU."""
        if isinstance(delay, bool) or not isinstance(delay, (int, np.integer)) or int(delay) < 0 \
                or (horizon is not None and int(delay) >= int(horizon)):
            raise ValueError("action delay must be an integer in [0, n_forwards%s), got %r" % ("" if horizon is None else " = %d" % horizon, delay))
        if action_dim is not None and not 1 <= int(action_dim) <= _lib.MAX_ACT_DIMS:
            raise ValueError("the actuator model holds up to %d action dims, got %r" % (_lib.MAX_ACT_DIMS, action_dim))
        prm = _lib.ActuatorParams()
        prm.delay, n_dims = int(delay), 0
        for name, val, default, field in (("rate_limit", rate_limit, math.inf, prm.rate_limit), ("rate_cost", rate_cost, 0.0, prm.rate_w)):
            try:
                arr = np.asarray(default if val is None else val, dtype=np.float32)
            except (TypeError, ValueError):
                raise ValueError("action %s must be a number or a list of them, got %r" % (name, val)) from None
            if arr.ndim > 1 or (arr.ndim == 1 and not 1 <= arr.shape[0] <= _lib.MAX_ACT_DIMS):
                raise ValueError("action %s must be a scalar or [A] with A <= %d, got shape %r" % (name, _lib.MAX_ACT_DIMS, arr.shape))
            if arr.ndim == 1:
                if (action_dim is not None and arr.shape[0] != int(action_dim)) or (n_dims and arr.shape[0] != n_dims):
                    raise ValueError("action %s has %d entries, expected %d (one per action dim)"
                                     % (name, arr.shape[0], n_dims if action_dim is None else int(action_dim)))
                n_dims = int(arr.shape[0])
            if name == "rate_limit" and not bool(np.all(arr > 0.0)):
                raise ValueError("action rate_limit must be > 0 (inf: no limit), got %r" % (val,))
            if name == "rate_cost" and not bool(np.all(np.isfinite(arr) & (arr >= 0.0))):
                raise ValueError("action rate_cost must be finite and >= 0, got %r" % (val,))
            full = np.full((_lib.MAX_ACT_DIMS,), arr if arr.ndim == 0 else default, dtype=np.float32)
            if arr.ndim == 1:
                full[:arr.shape[0]] = arr
            for k in range(_lib.MAX_ACT_DIMS):
                field[k] = float(full[k])
        prm.n_dims = n_dims
        return prm

    def _actuator_state(self, prev, prefix, m, d, who):
        """(prev [m,A], prefix [m,d,A]) float32 contiguous on the device, None staying None (unknown / nothing committed)"""
        if prev is not None:
            prev = self._t(prev)
            if tuple(prev.shape) != (m, self.A) or not prev.is_contiguous():
                raise ValueError("%s: prev %r, expected contiguous [%d,%d]" % (who, tuple(prev.shape), m, self.A))
        if prefix is not None:
            prefix = self._t(prefix)
            if tuple(prefix.shape) != (m, d, self.A) or not prefix.is_contiguous():
                raise ValueError("%s: prefix %r, expected contiguous [%d,%d,%d] (m, delay, A)" % (who, tuple(prefix.shape), m, d, self.A))
        return prev, prefix

    def actuate_actions(self, seqs, params, prev=None, prefix=None, want_cost=False):
        """`cadm_actuate_actions`: seqs [m,n,H,A] or [m,H,A] (a contiguous float32 device tensor) passed through the actuator model
        `params` (`actuator_params`) IN PLACE -- the committed steps of prefix [m,delay,A] pinned, every other step within the rate limits
        of the step before (step 0: of prev [m,A]) and the action box; NaN in prev / prefix, or None: unknown / not committed.  Returns
        seqs, with want_cost (seqs, cost [m,n] or [m]): sum_a sum_t w_a (u_t - u_{t-1})^2 of the actuated sequences."""
        if not isinstance(seqs, torch.Tensor) or seqs.dtype != torch.float32 or not seqs.is_contiguous() or seqs.dim() not in (3, 4) \
                or tuple(seqs.shape[-2:]) != (self.H, self.A) or seqs.shape[0] == 0 or not seqs.is_cuda:
            raise ValueError("actuate_actions: expected a contiguous float32 device tensor [m,n,%d,%d] or [m,%d,%d]" % (self.H, self.A, self.H, self.A))
        m, n = seqs.shape[0], seqs.shape[1] if seqs.dim() == 4 else 1
        prev, prefix = self._actuator_state(prev, prefix, m, params.delay, "actuate_actions")
        cost = torch.empty(tuple(seqs.shape[:-2]), dtype=torch.float32, device=self.device) if want_cost else None
        self._check(self.lib.cadm_actuate_actions(self._ctx, ct.byref(params), ptr(prev), ptr(prefix), m, n, ptr(seqs), ptr(cost), self.stream),
                    "cadm_actuate_actions")
        return (seqs, cost) if want_cost else seqs

    def actuated_plan(self, actuator, prev, prefix, advance, track, targets, offset, knots, phase, constraints, score, params, obs, cp_obs,
                      cp_act, init_mean, init_var, n, carry=None, carry_valid=None, seed=0, call=0, out=None, want_best_return=False):
        """`cadm_actuated_plan`: the loop of `tracking_plan` under the actuator model `actuator` (`actuator_params`; None = none, and
        `tracking_plan`'s launches): every iteration's candidates actuated behind the knot shaping, their rate cost taken off the candidate
        score, the plan actuated once more before it is written.  prev [m,A] / prefix [m,delay,A] (prefix may be None with delay 0): the
        envs' actuator state on the device, device tensors that `advance` moves on IN PLACE by one step behind the plan.  Arguments
        behind `advance` as `tracking_plan`; the workspace is the actuated slot (`cadm_actuated_workspace_bytes`)."""
        return self._nest_plan("actuated_plan", (actuator, prev, prefix, advance, track, targets, offset, knots, phase, constraints, score,
                               params), obs, cp_obs, cp_act, init_mean, init_var, n, carry, carry_valid, seed, call, out, want_best_return)

    # ------------------------------------------------------------------ pricing model uncertainty (opt-in; csrc/uncertainty.hip)
    @staticmethod
    def uncertainty_params(kind, weight, w=None, form="var", cap=None, obs_dim=None):
        """`cadm_uncertainty_params`: kind -- "epistemic" (the biased variance of the member means) or "total" (of the particles), a name
        or its CADM_UNC_* number; weight -- lambda, finite, any sign (> 0: a penalty on disagreement, < 0: a bonus); w -- None (1 for every
        dim), a scalar or [D]: the weight of each observation dim's variance, finite and >= 0 with at least one > 0 (dims with 0 are never
        read); form -- "var" (the weighted variance per step) or "std" (its square root); cap -- None (none) or a bound > 0 on the step
        cost.  An array must have `obs_dim` entries when that is given, at most `_lib.MAX_UNC_DIMS` anyway; the library checks it against
        the engine's D.  Needs no GPU."""
        def pick(val, table, what):
            if isinstance(val, str) and val in table:
                return table[val]
            if not isinstance(val, (bool, str)) and isinstance(val, (int, np.integer)) and int(val) in table.values():
                return int(val)
            raise ValueError("uncertainty %s must be %s, got %r" % (what, " or ".join(repr(k) for k in table), val))
        prm = _lib.UncertaintyParams()
        prm.kind, prm.form = pick(kind, _lib.UNC_KINDS, "kind"), pick(form, _lib.UNC_FORMS, "form")
        try:
            lam = float(np.float32(weight))
        except (TypeError, ValueError):
            raise ValueError("uncertainty weight must be a finite number, got %r" % (weight,)) from None
        if isinstance(weight, bool) or not math.isfinite(lam):
            raise ValueError("uncertainty weight must be a finite number, got %r" % (weight,))
        try:
            cp = math.inf if cap is None else float(np.float32(cap))
        except (TypeError, ValueError):
            raise ValueError("uncertainty cap must be None or a number > 0, got %r" % (cap,)) from None
        if not cp > 0.0:
            raise ValueError("uncertainty cap must be None or a number > 0, got %r" % (cap,))
        if obs_dim is not None and not 1 <= int(obs_dim) <= _lib.MAX_UNC_DIMS:
            raise ValueError("the uncertainty term holds up to %d observation dims, got %r" % (_lib.MAX_UNC_DIMS, obs_dim))
        try:
            arr = np.asarray(1.0 if w is None else w, dtype=np.float32)
        except (TypeError, ValueError):
            raise ValueError("uncertainty w must be None, a number or a list of them, got %r" % (w,)) from None
        if arr.ndim > 1 or (arr.ndim == 1 and not 1 <= arr.shape[0] <= _lib.MAX_UNC_DIMS):
            raise ValueError("uncertainty w must be a scalar or [D] with D <= %d, got shape %r" % (_lib.MAX_UNC_DIMS, arr.shape))
        if arr.ndim == 1 and obs_dim is not None and arr.shape[0] != int(obs_dim):
            raise ValueError("uncertainty w has %d entries, expected %d (one per observation dim)" % (arr.shape[0], int(obs_dim)))
        if not bool(np.all(np.isfinite(arr) & (arr >= 0.0))):
            raise ValueError("uncertainty w must be finite and >= 0, got %r" % (w,))
        if not bool(np.any(arr > 0.0)):
            raise ValueError("uncertainty w must be > 0 for at least one observation dim, got %r" % (w,))
        prm.weight, prm.cap, prm.n_dims = lam, cp, 0 if arr.ndim == 0 else int(arr.shape[0])
        full = np.zeros((_lib.MAX_UNC_DIMS,), np.float32)
        full[:max(1, prm.n_dims)] = arr
        for k in range(_lib.MAX_UNC_DIMS):
            prm.w[k] = float(full[k])
        return prm

    def uncertainty_cost(self, traj, params, first=None, want_steps=False):
        """`cadm_uncertainty_cost` on device tensors: traj [H,m,n,p,D] (a rollout's `traj_out`) -> cost [m,n], the step costs of
        `params` (`uncertainty_params`) added over the counted steps; with want_steps (step [m,n,H], cost): u_t of every step, counted
        or not.  first [m,n,p] int32 (None: every step counts): `constrain_returns`' first_violation -- steps behind the smallest one of a
        candidate's particles are not counted.  lambda is not applied."""
        traj, _, first, _ = HipEngine._returns_args(self, "uncertainty_cost", traj, None, first, None)
        H, m, n, p, D = traj.shape
        step = torch.empty((m, n, H), dtype=torch.float32, device=self.device) if want_steps else None
        cost = torch.empty((m, n), dtype=torch.float32, device=self.device)
        self._check(self.lib.cadm_uncertainty_cost(self._ctx, ct.byref(params), ptr(traj), ptr(first), m, n, ptr(step), ptr(cost), self.stream),
                    "cadm_uncertainty_cost")
        return (step, cost) if want_steps else cost

    def uncertain_plan(self, uncertainty, actuator, prev, prefix, advance, track, targets, offset, knots, phase, constraints, score, params, obs,
                       cp_obs, cp_act, init_mean, init_var, n, carry=None, carry_valid=None, seed=0, call=0, out=None, want_best_return=False):
        """`cadm_uncertain_plan`: the loop of `actuated_plan` with lambda times the uncertainty cost of `uncertainty`
        (`uncertainty_params`; None = none, and `actuated_plan`'s launches) taken off every iteration's candidate scores, behind the
        actuator's cost and before the refit.  Arguments behind `uncertainty` as `actuated_plan`; the workspace is the slot of
        `cadm_uncertain_workspace_bytes`, cached apart from the others."""
        return self._nest_plan("uncertain_plan", (uncertainty, actuator, prev, prefix, advance, track, targets, offset, knots, phase,
                               constraints, score, params), obs, cp_obs, cp_act, init_mean, init_var, n, carry, carry_valid, seed, call,
                               out, want_best_return)

    # ------------------------------------------------------------------ terminal value (opt-in; csrc/value.hip)
    @staticmethod
    def value_params(hidden_sizes=(), activation="relu", weight=1.0):
        """`cadm_value_params`: hidden_sizes -- the widths h_1 .. h_L of the value net D -> h_1 -> .. -> h_L -> 1, L in 0 ..
        `_lib.MAX_VALUE_LAYERS` (() is a linear V), each in 1 .. `_lib.MAX_VALUE_WIDTH`; activation -- "relu", "tanh" or "swish" (or its
        CADM_VALUE_* number), one for the net; weight -- what V is multiplied by before it is added to a return, finite (it carries a
        discount gamma^H -- not on an
        engine with `set_discount`: the library then multiplies gamma^H in).  Needs no GPU."""
        prm = _lib.ValueParams()
        HipEngine._net_params(prm, "value", hidden_sizes, activation, weight)
        return prm

    @staticmethod
    def _net_params(prm, what, hidden_sizes, activation, weight):
        """What `value_params`, `reward_params` and `policy_params` share: the checks of a caller-supplied net's layers, activation and
        weight, and the fields of `prm` (a `ValueParams`, a `RewardParams` or a `PolicyParams`) they fill."""
        try:
            hs = [hidden_sizes] if isinstance(hidden_sizes, (int, np.integer)) and not isinstance(hidden_sizes, bool) else list(hidden_sizes)
        except TypeError:
            raise ValueError("%s hidden_sizes must be a sequence of ints, got %r" % (what, hidden_sizes)) from None
        if len(hs) > _lib.MAX_VALUE_LAYERS:
            raise ValueError("a %s net has at most %d hidden layers, got %d" % (what, _lib.MAX_VALUE_LAYERS, len(hs)))
        for h in hs:
            if isinstance(h, bool) or not isinstance(h, (int, np.integer)) or not 1 <= int(h) <= _lib.MAX_VALUE_WIDTH:
                raise ValueError("a %s net's hidden widths must be ints in 1 .. %d, got %r" % (what, _lib.MAX_VALUE_WIDTH, h))
        if isinstance(activation, str) and activation in _lib.VALUE_ACTS:
            act = _lib.VALUE_ACTS[activation]
        elif not isinstance(activation, (bool, str)) and isinstance(activation, (int, np.integer)) and int(activation) in _lib.VALUE_ACTS.values():
            act = int(activation)
        else:
            raise ValueError("%s activation must be %s, got %r" % (what, " or ".join(repr(k) for k in _lib.VALUE_ACTS), activation))
        if weight is not None:      # (None: a net that is not added to a return -- the policy)
            try:
                w = float(np.float32(weight))
            except (TypeError, ValueError):
                raise ValueError("%s weight must be a finite number, got %r" % (what, weight)) from None
            if isinstance(weight, bool) or not math.isfinite(w):
                raise ValueError("%s weight must be a finite number, got %r" % (what, weight))
            prm.weight = w
        prm.n_hidden, prm.activation = len(hs), act
        for l, h in enumerate(hs):
            prm.hidden[l] = int(h)

    @staticmethod
    def value_weights(weights):
        """A value net's layers on the host: `weights` is a list of (W [in,out], b [out]) in numpy or torch, or a `torch.nn.Sequential` of
        `Linear` modules with `ReLU` / `Tanh` / `SiLU` between them (`Linear.weight` is [out,in]: transposed here).  Returns (the list of
        (W, b) as contiguous float32 numpy arrays, the activation's name or None when the input does not say).  Needs no GPU."""
        act = None
        if isinstance(weights, torch.nn.Module):
            if not isinstance(weights, torch.nn.Sequential):
                raise ValueError("a value net module must be a torch.nn.Sequential of Linear and ReLU / Tanh / SiLU modules, got %r" % (type(weights).__name__,))
            names = {torch.nn.ReLU: "relu", torch.nn.Tanh: "tanh", torch.nn.SiLU: "swish"}
            mods, pairs = list(weights), []
            if not mods or len(mods) % 2 == 0:
                raise ValueError("a value net Sequential alternates Linear and activation modules and ends with a Linear (got %d modules)" % len(mods))
            for j, mod in enumerate(mods):
                if j % 2 == 0:
                    if not isinstance(mod, torch.nn.Linear) or mod.bias is None:
                        raise ValueError("value net Sequential: module %d must be a Linear with a bias, got %r" % (j, type(mod).__name__))
                    pairs.append((mod.weight.detach().t(), mod.bias.detach()))
                else:
                    if type(mod) not in names:
                        raise ValueError("value net Sequential: module %d must be ReLU, Tanh or SiLU, got %r" % (j, type(mod).__name__))
                    if act is not None and names[type(mod)] != act:
                        raise ValueError("value net Sequential: one activation for the whole net, got %r and %r" % (act, names[type(mod)]))
                    act = names[type(mod)]
            weights = pairs
        try:
            items = [(w, b) for w, b in weights]
        except (TypeError, ValueError):
            raise ValueError("value net weights must be a list of (W [in,out], b [out]) pairs or a torch.nn.Sequential") from None
        out = []
        for l, (w, b) in enumerate(items):
            w = w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else np.asarray(w)
            b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
            w, b = np.ascontiguousarray(w, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
            if w.ndim != 2 or b.ndim != 1 or b.shape[0] != w.shape[1]:
                raise ValueError("value net layer %d: W %r and b %r, expected [in,out] and [out]" % (l, w.shape, b.shape))
            if not (np.all(np.isfinite(w)) and np.all(np.isfinite(b))):
                raise ValueError("value net layer %d holds a weight or a bias that is not finite" % l)
            out.append((w, b))
        return out, act

    def set_value_net(self, params, weights=None, obs_mean=None, obs_std=None):
        """`cadm_set_value_net`: registers the value net that `params` (`value_params`) describes -- `weights` as `value_weights` takes
        them, the input statistics obs_mean / obs_std [D] (None: 0 / 1; std finite and > 0; 1 / std is formed in float64 and rounded once
        to float32).  Shapes and finiteness are checked here; the library packs a copy of its own, so a second call replaces the net
        without touching anything else.  params None: the net is cleared."""
        self._value_src = HipEngine._set_net(self, "set_value_net", params, self.D, weights, obs_mean, obs_std, "obs_mean", "obs_std")

    def _set_net(self, who, params, K, weights, mean, std, mean_name, std_name, N=1):
        """What `set_value_net`, `set_reward_net` and `set_policy_net` share (and, piece by piece, `set_critic_nets`): the checks of a
        caller-supplied net K -> hidden -> N against its declared `params` and of its input statistics [K] -- all of them before the
        library is looked at --, the staging, and the call of cadm_<who>.  Returns what must stay alive until the next net; params
        None: the net is cleared, and None."""
        if params is None:
            self._check(getattr(self.lib, "cadm_" + who)(self._ctx, None, None, None, None, None, self.stream), "cadm_" + who)
            return None
        layers = HipEngine._net_layers(self, who, params, weights, K, N)
        mean, std = HipEngine._net_stats(self, who, K, mean, std, mean_name, std_name)
        return HipEngine._net_register(self, who, params, layers, mean, std)

    def _net_layers(self, who, params, weights, K, N, critic=None):
        """The layers [(W, b)] of one caller-supplied net (`value_weights`) checked against the declared K -> hidden -> N of `params`;
        critic: its index among the nets of `set_critic_nets`, which the messages then name."""
        layers, act = self.value_weights(weights)
        dims = [K] + [int(params.hidden[l]) for l in range(params.n_hidden)] + [N]
        if len(layers) != len(dims) - 1:
            given = "%d layers given" % len(layers) if critic is None else "critic %d has %d layers" % (critic, len(layers))
            raise ValueError("%s: %s, the declared net %r has %d" % (who, given, dims, len(dims) - 1))
        for l, (w, b) in enumerate(layers):
            if w.shape != (dims[l], dims[l + 1]):
                which = "layer %d" % l if critic is None else "layer %d of critic %d" % (l, critic)
                raise ValueError("%s: %s is %r, the declared net %r needs %r" % (who, which, w.shape, dims, (dims[l], dims[l + 1])))
        if act is not None and _lib.VALUE_ACTS[act] != params.activation:
            whose = "the module's activation %r" % (act,) if critic is None else "the activation %r of critic %d's module" % (act, critic)
            raise ValueError("%s: %s is not the declared one" % (who, whose))
        return layers

    def _net_stats(self, who, K, mean, std, mean_name, std_name):
        """The input statistics [K] of a caller-supplied net in float64 (None: 0 / 1), checked."""
        mean = np.zeros((K,), np.float64) if mean is None else np.asarray(self._host(mean), dtype=np.float64).reshape(-1)
        std = np.ones((K,), np.float64) if std is None else np.asarray(self._host(std), dtype=np.float64).reshape(-1)
        if mean.shape != (K,) or std.shape != (K,):
            raise ValueError("%s: %s %r / %s %r, expected [%d]" % (who, mean_name, mean.shape, std_name, std.shape, K))
        if not np.all(np.isfinite(mean)):
            raise ValueError("%s: %s must be finite" % (who, mean_name))
        if not np.all(np.isfinite(std) & (std > 0.0)):
            raise ValueError("%s: %s must be finite and > 0" % (who, std_name))
        return mean, std

    def _net_register(self, who, params, layers, mean, std):
        """Stages the checked layers (of every net, net by net) and statistics and calls cadm_<who>; returns what must stay alive until
        the next registration (the copy is enqueued, not done)."""
        dev = [(self._t(w), self._t(b)) for w, b in layers]
        mean_d, inv_d = self._t(mean.astype(np.float32)), self._t((1.0 / std).astype(np.float32))
        nl = len(dev)
        Wp, bp = (ct.c_void_p * nl)(*[w.data_ptr() for w, _ in dev]), (ct.c_void_p * nl)(*[b.data_ptr() for _, b in dev])
        self._check(getattr(self.lib, "cadm_" + who)(self._ctx, ct.byref(params), Wp, bp, ptr(mean_d), ptr(inv_d), self.stream), "cadm_" + who)
        return (dev, mean_d, inv_d)

    @staticmethod
    def _host(x):
        return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x

    def _flat_rows(self, who, x, K, name="states", none="no states"):
        """What the nets' `*_eval` share: x [..., K] as a device tensor and flattened to [R, K], R >= 1."""
        x = self._t(x)
        if x.dim() < 1 or x.shape[-1] != K:
            raise ValueError("%s: %s %r, expected [..., %d]" % (who, name, tuple(x.shape), K))
        flat = x.reshape(-1, K).contiguous()
        if flat.shape[0] < 1:
            raise ValueError("%s: %s" % (who, none))
        return x, flat

    def _returns_args(self, who, traj, rows, first, out):
        """What the stand-alone stage calls behind a rollout share: traj [H,m,n,p,D] and rows [m,n,p] as checked device tensors, first
        [m,n,p] int32 or None, and out [m,n,p] (None: a new tensor).  rows None (`uncertainty_cost` reads none): no rows, no out."""
        traj = self._t(traj)
        if traj.dim() != 5:
            raise ValueError("%s: traj %r: expected contiguous [H,m,n,p,D]" % (who, tuple(traj.shape)))
        H, m, n, p, D = traj.shape
        if (H, p, D) != (self.H, self.p, self.D):
            raise ValueError("%s: traj %r does not agree with the engine (H=%d, p=%d, D=%d)" % (who, tuple(traj.shape), self.H, self.p, self.D))
        if rows is not None:
            rows = self._t(rows)
            if tuple(rows.shape) != (m, n, p):
                raise ValueError("%s: rows %r, expected contiguous %r" % (who, tuple(rows.shape), (m, n, p)))
        if first is not None:
            first = self._t(first, dtype=torch.int32)
            if tuple(first.shape) != (m, n, p):
                raise ValueError("%s: first %r, expected contiguous int32 %r" % (who, tuple(first.shape), (m, n, p)))
        if rows is None:
            return traj, None, first, None
        if out is None:
            out = torch.empty_like(rows)
        elif tuple(out.shape) != (m, n, p) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != rows.device:
            raise ValueError("%s: out must be a contiguous float32 device tensor %r" % (who, (m, n, p)))
        return traj, rows, first, out

    def value_eval(self, states):
        """`cadm_value_eval`: V of states [..., D] -> [...] (device tensors), through the planner's kernel."""
        states, flat = HipEngine._flat_rows(self, "value_eval", states, self.D)
        v = torch.empty((flat.shape[0],), dtype=torch.float32, device=self.device)
        self._check(self.lib.cadm_value_eval(self._ctx, ptr(flat), int(flat.shape[0]), ptr(v), self.stream), "cadm_value_eval")
        return v.reshape(states.shape[:-1])

    def value_returns(self, traj, rows, params, first=None, want_v=False, out=None):
        """`cadm_value_returns` on device tensors: traj [H,m,n,p,D] (a rollout's `traj_out`), rows [m,n,p] -> rows + weight * V(traj[H-1])
        per row under `params` (`value_params`, describing the registered net).  first [m,n,p] int32 (None: every row):
        `constrain_returns`' first_violation -- a row with first < H keeps its bits.  want_v: (rows_out, v [m,n,p]), v NaN where skipped.
        out: where the new rows go (may be `rows` itself)."""
        traj, rows, first, out = HipEngine._returns_args(self, "value_returns", traj, rows, first, out)
        H, m, n, p, D = traj.shape
        v = torch.empty((m, n, p), dtype=torch.float32, device=self.device) if want_v else None
        self._check(self.lib.cadm_value_returns(self._ctx, ct.byref(params), ptr(traj), ptr(first), m, n, ptr(rows), ptr(out), ptr(v),
                                                self.stream), "cadm_value_returns")
        return (out, v) if want_v else out

    def valued_plan(self, value, uncertainty, actuator, prev, prefix, advance, track, targets, offset, knots, phase, constraints, score, params,
                    obs, cp_obs, cp_act, init_mean, init_var, n, carry=None, carry_valid=None, seed=0, call=0, out=None, want_best_return=False):
        """`cadm_valued_plan`: the loop of `uncertain_plan` with `value.weight` times the registered value net's V of every particle's last
        state added to the particle returns, behind the constraints and the tracking terms and before the score (`value`: a
        `value_params` describing the net of `set_value_net`; None = none, and `uncertain_plan`'s launches).  Arguments behind `value` as
        `uncertain_plan`; the workspace is the slot of `cadm_valued_workspace_bytes`, cached apart from the others."""
        return self._nest_plan("valued_plan", (value, uncertainty, actuator, prev, prefix, advance, track, targets, offset, knots, phase,
                               constraints, score, params), obs, cp_obs, cp_act, init_mean, init_var, n, carry, carry_valid, seed, call,
                               out, want_best_return)

    # ------------------------------------------------------------------ learned reward (opt-in; csrc/reward.hip)
    @staticmethod
    def reward_params(inputs="obs_act_next_obs", hidden_sizes=(), activation="relu", weight=1.0):
        """`cadm_reward_params`: inputs -- what the reward net reads per step: "next_obs" (s_{t+1}; K = D), "obs_act" (s_t, a_t; K = D + A)
        or "obs_act_next_obs" (s_t, a_t, s_{t+1}; K = 2 D + A), or its CADM_REWARD_* number; hidden_sizes / activation / weight -- as
        `value_params` (the net is K -> h_1 -> .. -> h_L -> 1; weight is what the step sum is multiplied by before it is added to a
        return).  Needs no GPU."""
        if isinstance(inputs, str) and inputs in _lib.REWARD_INPUTS:
            inp = _lib.REWARD_INPUTS[inputs]
        elif not isinstance(inputs, (bool, str)) and isinstance(inputs, (int, np.integer)) and int(inputs) in _lib.REWARD_INPUTS.values():
            inp = int(inputs)
        else:
            raise ValueError("reward inputs must be %s, got %r" % (" or ".join(repr(k) for k in _lib.REWARD_INPUTS), inputs))
        prm = _lib.RewardParams()
        HipEngine._net_params(prm, "reward", hidden_sizes, activation, weight)
        prm.inputs = inp
        return prm

    @staticmethod
    def reward_input_dims(inputs, D, A):
        """K of a reward net on D observation and A action dims; inputs: a name or a CADM_REWARD_* number."""
        inp = _lib.REWARD_INPUTS[inputs] if isinstance(inputs, str) else int(inputs)
        return (D, D + A, 2 * D + A)[inp]

    def set_reward_net(self, params, weights=None, in_mean=None, in_std=None):
        """`cadm_set_reward_net`: registers the reward net that `params` (`reward_params`) describes -- `weights` as `value_weights` takes
        them, the input statistics in_mean / in_std [K] over the concatenated input (None: 0 / 1; std finite and > 0; 1 / std is formed
        in float64 and rounded once to float32).  Shapes and finiteness are checked here; the library packs a copy of its own, so a second
        call replaces the net without touching anything else.  params None: the net is cleared."""
        K = None if params is None else HipEngine.reward_input_dims(params.inputs, self.D, self.A)
        self._reward_src = HipEngine._set_net(self, "set_reward_net", params, K, weights, in_mean, in_std, "in_mean", "in_std")
        self._reward_K = K

    def reward_eval(self, x):
        """`cadm_reward_eval`: R of already concatenated inputs x [..., K] -> [...] (device tensors), through the planner's kernel."""
        x = self._t(x)
        K = getattr(self, "_reward_K", None)
        if K is None:
            raise _lib.CadmError("reward_eval: no reward net is registered (call set_reward_net)")
        x, flat = HipEngine._flat_rows(self, "reward_eval", x, K, "x", "no inputs")
        r = torch.empty((flat.shape[0],), dtype=torch.float32, device=self.device)
        self._check(self.lib.cadm_reward_eval(self._ctx, ptr(flat), int(flat.shape[0]), ptr(r), self.stream), "cadm_reward_eval")
        return r.reshape(x.shape[:-1])

    def reward_returns(self, traj, obs, actions, rows, params, first=None, want_steps=False, out=None):
        """`cadm_reward_returns` on device tensors: traj [H,m,n,p,D] (a rollout's `traj_out`), obs [m,D], actions [m,n,H,A] (what the
        rollout read), rows [m,n,p] -> rows + weight * S per row under `params` (`reward_params`, describing the registered net), S the
        sum of R over the counted steps in ascending t.  first [m,n,p] int32 (None: every step counts): `constrain_returns`'
        first_violation -- the steps t <= first count.  want_steps: (rows_out, steps [H,m,n,p], S [m,n,p]), steps NaN where not counted;
        else the step rewards go to a cached workspace.  out: where the new rows go (may be `rows` itself).  Of several bad arguments
        traj, rows, first and out are refused before obs and actions (`_returns_args` runs first)."""
        traj, rows, first, out = HipEngine._returns_args(self, "reward_returns", traj, rows, first, out)
        H, m, n, p, D = traj.shape
        obs, actions = self._t(obs), self._t(actions)
        if tuple(obs.shape) != (m, D):
            raise ValueError("reward_returns: obs %r, expected contiguous %r" % (tuple(obs.shape), (m, D)))
        if tuple(actions.shape) != (m, n, H, self.A):
            raise ValueError("reward_returns: actions %r, expected contiguous %r" % (tuple(actions.shape), (m, n, H, self.A)))
        steps = S = ws = None
        if want_steps:
            steps = torch.empty((H, m, n, p), dtype=torch.float32, device=self.device)
            S = torch.empty((m, n, p), dtype=torch.float32, device=self.device)
        else:
            need = self.lib.cadm_reward_workspace_bytes(self._ctx, m, n)
            ws = getattr(self, "_reward_ws", None)
            if ws is None or ws.numel() < need:
                ws = self._reward_ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=self.device)
        self._check(self.lib.cadm_reward_returns(self._ctx, ct.byref(params), ptr(traj), ptr(obs), ptr(actions), ptr(first), m, n, ptr(rows),
                                                 ptr(out), ptr(steps), ptr(S), ptr(ws), self.stream), "cadm_reward_returns")
        return (out, steps, S) if want_steps else out

    def rewarded_plan(self, reward, value, uncertainty, actuator, prev, prefix, advance, track, targets, offset, knots, phase, constraints,
                      score, params, obs, cp_obs, cp_act, init_mean, init_var, n, carry=None, carry_valid=None, seed=0, call=0, out=None,
                      want_best_return=False):
        """`cadm_rewarded_plan`: the loop of `valued_plan` with `reward.weight` times the registered reward net's step sum added to the
        particle returns, behind the constraints and the tracking terms and in front of the terminal value (`reward`: a `reward_params`
        describing the net of `set_reward_net`; None = none, and `valued_plan`'s launches).  Arguments behind `reward` as `valued_plan`;
        the workspace is the slot of `cadm_rewarded_workspace_bytes`, cached apart from the others."""
        return self._nest_plan("rewarded_plan", (reward, value, uncertainty, actuator, prev, prefix, advance, track, targets, offset, knots,
                               phase, constraints, score, params), obs, cp_obs, cp_act, init_mean, init_var, n, carry, carry_valid, seed,
                               call, out, want_best_return)

    # ------------------------------------------------------------------ policy prior (opt-in; csrc/policy.hip)
    @staticmethod
    def policy_params(hidden_sizes=(), activation="relu", squash="tanh", n_samples=1, noise_std=0.0):
        """`cadm_policy_params`: hidden_sizes / activation -- as `value_params` (the net is D -> h_1 -> .. -> h_L -> A); squash -- "tanh"
        (a = mid + half * tanh(z), onto the action bounds) or "none" (a = z), or its CADM_POLICY_* number; n_samples -- P >= 1, the
        proposal sequences per env; noise_std -- finite, >= 0, the exploration noise of sequences 1 .. P - 1 (sequence 0 is the policy's
        own trajectory).  Needs no GPU."""
        if isinstance(squash, str) and squash in _lib.POLICY_SQUASH:
            sq = _lib.POLICY_SQUASH[squash]
        elif not isinstance(squash, (bool, str)) and isinstance(squash, (int, np.integer)) and int(squash) in _lib.POLICY_SQUASH.values():
            sq = int(squash)
        else:
            raise ValueError("policy squash must be %s, got %r" % (" or ".join(repr(k) for k in _lib.POLICY_SQUASH), squash))
        if isinstance(n_samples, bool) or not isinstance(n_samples, (int, np.integer)) or int(n_samples) < 1:
            raise ValueError("policy n_samples must be an int >= 1, got %r" % (n_samples,))
        try:
            std = float(np.float32(noise_std))
        except (TypeError, ValueError):
            raise ValueError("policy noise_std must be a finite number >= 0, got %r" % (noise_std,)) from None
        if isinstance(noise_std, bool) or not math.isfinite(std) or std < 0.0:
            raise ValueError("policy noise_std must be a finite number >= 0, got %r" % (noise_std,))
        prm = _lib.PolicyParams()
        HipEngine._net_params(prm, "policy", hidden_sizes, activation, None)
        prm.squash, prm.n_samples, prm.noise_std = sq, int(n_samples), std
        return prm

    def set_policy_net(self, params, weights=None, obs_mean=None, obs_std=None):
        """`cadm_set_policy_net`: registers the policy net that `params` (`policy_params`) describes -- `weights` as `value_weights` takes
        them (the last layer has A outputs), the input statistics obs_mean / obs_std [D] as `set_value_net` takes them.  The library
        packs a copy of its own, so a second call replaces the net without touching anything else.  params None: the net is cleared."""
        self._policy_src = HipEngine._set_net(self, "set_policy_net", params, self.D, weights, obs_mean, obs_std, "obs_mean", "obs_std", N=self.A)

    def policy_eval(self, states):
        """`cadm_policy_eval`: the registered policy's action of states [..., D] -> [..., A] (device tensors): squash and clip, no
        noise, through the chain of the proposal roll."""
        states, flat = HipEngine._flat_rows(self, "policy_eval", states, self.D)
        a = torch.empty((flat.shape[0], self.A), dtype=torch.float32, device=self.device)
        self._check(self.lib.cadm_policy_eval(self._ctx, ptr(flat), int(flat.shape[0]), ptr(a), self.stream), "cadm_policy_eval")
        return a.reshape(tuple(states.shape[:-1]) + (self.A,))

    def set_policy_head(self, params, W_ls=None, b_ls=None):
        """`cadm_set_policy_head`: the Gaussian head of the registered policy net -- `params` a `_lib.PolicyHeadParams`
        (`planner.policy_head_params`), W_ls [h_L, A] (a linear policy: [D, A]) and b_ls [A] the log-std layer on the net's last hidden
        layer, numpy or torch, finite.  The library packs a copy of its own; `set_policy_net` drops the head.  params None: cleared."""
        if params is None:
            self._check(self.lib.cadm_set_policy_head(self._ctx, None, None, None, self.stream), "cadm_set_policy_head")
            self._policy_head_src = None
            return
        W = np.ascontiguousarray(self._host(W_ls), dtype=np.float32)
        b = np.ascontiguousarray(self._host(b_ls), dtype=np.float32)
        if W.ndim != 2 or W.shape[1] != self.A or b.shape != (self.A,):
            raise ValueError("set_policy_head: W_ls %r and b_ls %r, expected [h_L, %d] and [%d]" % (W.shape, b.shape, self.A, self.A))
        src = getattr(self, "_policy_src", None)
        if src is not None and tuple(src[0][-1][0].shape)[0] != W.shape[0]:
            raise ValueError("set_policy_head: W_ls has %d rows, the registered net's last layer reads %d" % (W.shape[0], src[0][-1][0].shape[0]))
        if not (np.all(np.isfinite(W)) and np.all(np.isfinite(b))):
            raise ValueError("set_policy_head: the log-std layer holds a weight or a bias that is not finite")
        Wd, bd = self._t(W), self._t(b)
        self._check(self.lib.cadm_set_policy_head(self._ctx, ct.byref(params), ptr(Wd), ptr(bd), self.stream), "cadm_set_policy_head")
        self._policy_head_src = (Wd, bd)      # (the copy is enqueued, not done)

    @staticmethod
    def policy_proposals_args(source="noise", std_scale=1.0):
        """What `set_policy_proposals` takes, checked -> (the CADM_PROPOSE_* number, std_scale as the float32 the library is handed):
        source "noise" | "head"; std_scale a finite number >= 0, no bool.  Needs no GPU."""
        if not isinstance(source, str) or source not in _lib.PROPOSALS:
            raise ValueError("policy proposals must be %s, got %r" % (" or ".join(repr(k) for k in _lib.PROPOSALS), source))
        if isinstance(std_scale, (bool, np.bool_)) or not isinstance(std_scale, (int, float, np.integer, np.floating)):
            raise ValueError("policy std_scale must be a finite number >= 0, got %r" % (std_scale,))
        scale = float(np.float32(std_scale))
        if not math.isfinite(scale) or scale < 0.0:
            raise ValueError("policy std_scale must be a finite number >= 0, got %r" % (std_scale,))
        return _lib.PROPOSALS[source], scale

    def set_policy_proposals(self, source="noise", std_scale=1.0):
        """`cadm_set_policy_proposals`: where sequences 1 .. P - 1 of `policy_propose` (and of `guided_plan` / `critic_plan`) come from --
        "noise": the mode action plus the call's noise_std (the default); "head": draws of the registered net's Gaussian head
        (`set_policy_head`) at std_scale times the standard deviation it predicts at every state.  State of the engine, as the discount
        is: it survives `set_policy_net` and `set_policy_head`."""
        src, scale = HipEngine.policy_proposals_args(source, std_scale)
        self._check(self.lib.cadm_set_policy_proposals(self._ctx, src, scale), "cadm_set_policy_proposals")

    def policy_sample(self, states, row0=0, t=0, seed=0, call=0):
        """`cadm_policy_sample`: states [..., D] -> dict(act [..., A], logp [...], mode [..., A]) (device tensors): an action drawn from
        the registered net's Gaussian head, its log-density, and `policy_eval`'s action.  Flattened row r draws as row row0 + r of step
        t under the Philox key (seed, call)."""
        states, flat = HipEngine._flat_rows(self, "policy_sample", states, self.D)
        R = int(flat.shape[0])
        act = torch.empty((R, self.A), dtype=torch.float32, device=self.device)
        mode = torch.empty((R, self.A), dtype=torch.float32, device=self.device)
        logp = torch.empty((R,), dtype=torch.float32, device=self.device)
        self._check(self.lib.cadm_policy_sample(self._ctx, ptr(flat), R, int(row0), int(t), seed, call, ptr(act), ptr(logp), ptr(mode),
                                                self.stream), "cadm_policy_sample")
        lead = tuple(states.shape[:-1])
        return dict(act=act.reshape(lead + (self.A,)), logp=logp.reshape(lead), mode=mode.reshape(lead + (self.A,)))

    def policy_propose(self, params, obs, ctx_vec=None, seed=0, call=0, want_states=False):
        """`cadm_policy_propose`: obs [m,D], ctx_vec the context encoder's output (`context_forward`; None for a model without one) ->
        the P = params.n_samples proposal sequences per env [m,P,H,A]: the registered policy rolled through the model on the particle
        mean of every sequence, sequence 0 without noise.  want_states: (seqs, states [H,m,P,p,D]), the particle states every step
        read."""
        obs = self._t(obs)
        if obs.dim() != 2 or obs.shape[1] != self.D or not obs.is_contiguous():
            raise ValueError("policy_propose: obs %r, expected contiguous [m, %d]" % (tuple(obs.shape), self.D))
        m, P = int(obs.shape[0]), int(params.n_samples)
        ctx_vec = None if ctx_vec is None else self._t(ctx_vec)
        if P >= 1:
            self.ensure_rollout(None, m, P)
        seqs = torch.empty((m, max(P, 1), self.H, self.A), dtype=torch.float32, device=self.device)
        states = torch.empty((self.H, m, max(P, 1), self.p, self.D), dtype=torch.float32, device=self.device) if want_states else None
        need = self.lib.cadm_policy_workspace_bytes(self._ctx, m, max(P, 1))
        ws = getattr(self, "_policy_ws", None)
        if ws is None or ws.numel() < need:
            ws = self._policy_ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=self.device)
        self._check(self.lib.cadm_policy_propose(self._ctx, ct.byref(params), ptr(obs), ptr(ctx_vec), m, seed, call, ptr(seqs), ptr(states),
                                                 ptr(ws), self.stream), "cadm_policy_propose")
        return (seqs, states) if want_states else seqs

    def _imagine_w(self, w):
        """the disagreement weights of `imagine` / `imagine_select` as the library takes them: None (w = 1), or an `UncertaintyParams`
        holding [D] weights (only n_dims and w are read)"""
        if w is None or isinstance(w, _lib.UncertaintyParams):
            return w
        return HipEngine.uncertainty_params("epistemic", 1.0, w, "var", None, obs_dim=self.D)

    def imagine(self, obs, ctx_vec=None, horizon=1, branches=1, actions=None, noise_std=0.0, constraints=None, w=None, seed=0, call=0,
                sample=False):
        """`cadm_imagine`: n = branches rollouts of k = horizon one-step rollouts from each of obs [m,D] (ctx_vec: the context encoder's
        output for them, None without one), under actions [m,n,k,A] (raw, clipped) or, with None, the registered policy net perturbed by
        noise_std * xi on every row -> a dict of device tensors, views of ONE buffer the call allocates: states [k+1,m,n,D], act
        [k,m,n,A], rew [k,m,n], done / valid [k,m,n] uint8, member [k,m,n] int32, disagreement [k,m,n], length [m,n] int32, alive [m,n]
        uint8.  constraints: a `ConstraintParams` (a violated one ends the row) or None; w: None, [D] weights or an
        `UncertaintyParams` of the disagreement.  (seed, call): the Philox key of the head noise, the particle draws and the action noise.
        sample: `cadm_imagine_sampled` -- the actions are drawn from the registered net's Gaussian head (`set_policy_head`; no actions,
        no noise_std), and the dict also holds logp [k,m,n], the log-density of act[t,row] at states[t,row]."""
        if sample and (actions is not None or float(noise_std) != 0.0):
            raise ValueError("imagine: sample=True takes neither actions nor a noise_std")
        obs = self._t(obs)
        if obs.dim() != 2 or obs.shape[1] != self.D or not obs.is_contiguous():
            raise ValueError("imagine: obs %r, expected contiguous [m, %d]" % (tuple(obs.shape), self.D))
        m, n, k = int(obs.shape[0]), int(branches), int(horizon)
        if actions is not None:
            actions = self._t(actions)
            if tuple(actions.shape) != (m, n, k, self.A):
                raise ValueError("imagine: actions %r, expected %r" % (tuple(actions.shape), (m, n, k, self.A)))
        ctx_vec = None if ctx_vec is None else self._t(ctx_vec)
        w = self._imagine_w(w)
        if m >= 1 and n >= 1:
            self.ensure_rollout(None, m, n)
        cons, wref = None if constraints is None else ct.byref(constraints), None if w is None else ct.byref(w)
        if sample:
            off = (ct.c_uint64 * _lib.IMAGINE_SAMPLED_VIEWS)()
            need = self.lib.cadm_imagine_sampled_workspace_bytes(self._ctx, m, n, k, off)
            buf = torch.empty((max(int(need), 1),), dtype=torch.uint8, device=self.device)
            self._check(self.lib.cadm_imagine_sampled(self._ctx, ptr(obs), ptr(ctx_vec), m, n, k, cons, wref, seed, call, ptr(buf), self.stream),
                        "cadm_imagine_sampled")
        else:
            off = (ct.c_uint64 * _lib.IMAGINE_VIEWS)()
            need = self.lib.cadm_imagine_workspace_bytes(self._ctx, m, n, k, off)
            buf = torch.empty((max(int(need), 1),), dtype=torch.uint8, device=self.device)
            self._check(self.lib.cadm_imagine(self._ctx, ptr(obs), ptr(ctx_vec), ptr(actions), m, n, k, float(noise_std), cons, wref,
                                              seed, call, ptr(buf), self.stream), "cadm_imagine")
        views = (("states", torch.float32, (k + 1, m, n, self.D)), ("act", torch.float32, (k, m, n, self.A)), ("rew", torch.float32, (k, m, n)),
                 ("done", torch.uint8, (k, m, n)), ("valid", torch.uint8, (k, m, n)), ("member", torch.int32, (k, m, n)),
                 ("disagreement", torch.float32, (k, m, n)), ("length", torch.int32, (m, n)), ("alive", torch.uint8, (m, n)))
        if sample:
            views += (("logp", torch.float32, (k, m, n)),)
        out = {}
        for (name, dtype, shape), o in zip(views, off):
            nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            out[name] = buf[int(o):int(o) + nbytes].view(dtype).view(shape)
        return out

    def imagine_select(self, nxt, rows1, state, alive, t=0, sel=None, constraints=None, w=None, seed=0, call=0, length=None, want_bcast=True):
        """`cadm_imagine_select`, the stage between two of `imagine`'s rollouts alone: nxt [R,p,D] and rows1 [R,p] (a one-step rollout's
        states and returns), state [R,D] (states[t]), alive [R] uint8 -> dict(state, rew, done, valid, member, disagreement, alive, length,
        bcast): the outputs of step t for the R rows; `alive` and `length` (None: zeros) are copied, not changed.  sel [R] int32: the
        particle of every row in the place of the draw under (seed, call, row, t)."""
        nxt, rows1, state = self._t(nxt), self._t(rows1), self._t(state)
        R = int(state.shape[0]) if state.dim() == 2 else -1
        if tuple(nxt.shape) != (R, self.p, self.D) or tuple(rows1.shape) != (R, self.p) or tuple(state.shape) != (R, self.D) or R < 1:
            raise ValueError("imagine_select: next %r, rows1 %r, state %r: expected [R,%d,%d], [R,%d], [R,%d]"
                             % (tuple(nxt.shape), tuple(rows1.shape), tuple(state.shape), self.p, self.D, self.p, self.D))
        alive = self._t(alive, dtype=torch.uint8).clone()
        length = torch.zeros((R,), dtype=torch.int32, device=self.device) if length is None else self._t(length, dtype=torch.int32).clone()
        sel = None if sel is None else self._t(sel, dtype=torch.int32)
        if tuple(alive.shape) != (R,) or tuple(length.shape) != (R,) or (sel is not None and tuple(sel.shape) != (R,)):
            raise ValueError("imagine_select: alive / length / sel must be [%d]" % R)
        w = self._imagine_w(w)
        new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=self.device)
        out = dict(state=new((R, self.D)), rew=new((R,)), done=new((R,), torch.uint8), valid=new((R,), torch.uint8),
                   member=new((R,), torch.int32), disagreement=new((R,)), alive=alive, length=length,
                   bcast=new((R, self.p, self.D)) if want_bcast else None)
        self._check(self.lib.cadm_imagine_select(self._ctx, ptr(nxt), ptr(rows1), ptr(state), ptr(sel), R, int(t),
                                                 None if constraints is None else ct.byref(constraints), None if w is None else ct.byref(w),
                                                 seed, call, ptr(alive), ptr(out["state"]), ptr(out["rew"]), ptr(out["done"]), ptr(out["valid"]),
                                                 ptr(out["member"]), ptr(out["disagreement"]), ptr(length), ptr(out["bcast"]), self.stream),
                    "cadm_imagine_select")
        return out

    def imagine_targets(self, rew, valid, done, disagreement, boot, gamma, lam=0.95, penalty=0.0, max_disagreement=None, steve_var_floor=None):
        """`cadm_imagine_targets`: rew, disagreement [k,m,n] float32, valid, done [k,m,n] uint8 (`imagine`'s outputs) and boot [k+1,m,n],
        the bootstrap value of states[t] -- device tensors, read only -> a dict of device tensors, views of ONE buffer the call allocates:
        lambda_return, nstep [k,m,n], nstep_ok, used [k,m,n] uint8 and, with steve_var_floor (a finite number > 0), steve [m],
        steve_weight, steve_mean, steve_var [k,m], steve_count [k,m] int32, steve_fallback [m] uint8.  gamma, lam, penalty,
        max_disagreement (None: no bound): include/cadm_hip.h "Value-expansion targets"; the library refuses what is out of range."""
        k, m, n = (int(v) for v in rew.shape) if isinstance(rew, torch.Tensor) and rew.dim() == 3 else (-1, -1, -1)
        for name, t, dtype, shape in (("rew", rew, torch.float32, (k, m, n)), ("valid", valid, torch.uint8, (k, m, n)),
                                      ("done", done, torch.uint8, (k, m, n)), ("disagreement", disagreement, torch.float32, (k, m, n)),
                                      ("boot", boot, torch.float32, (k + 1, m, n))):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()) or k < 1 or tuple(t.shape) != shape:
                raise ValueError("imagine_targets: %s must be a contiguous %s device tensor %s, got %s"
                                 % (name, str(dtype).split(".")[-1], "[k,m,n]" if name == "rew" else list(shape),
                                    "%r %s" % (tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__))
        steve = steve_var_floor is not None
        prm = _lib.TargetParams(float(gamma), float(lam), float(penalty), float("inf") if max_disagreement is None else float(max_disagreement),
                                float(steve_var_floor) if steve else 0.0, int(steve))
        off = (ct.c_uint64 * _lib.TARGET_VIEWS)()
        need = self.lib.cadm_imagine_targets_workspace_bytes(self._ctx, m, n, k, int(steve), off)
        buf = torch.empty((max(int(need), 1),), dtype=torch.uint8, device=self.device)      # (need 0: the call below says what is refused)
        self._check(self.lib.cadm_imagine_targets(self._ctx, ptr(rew), ptr(valid), ptr(done), ptr(disagreement), ptr(boot), m, n, k,
                                                  ct.byref(prm), ptr(buf), self.stream), "cadm_imagine_targets")
        views = [("lambda_return", torch.float32, (k, m, n)), ("nstep", torch.float32, (k, m, n)), ("nstep_ok", torch.uint8, (k, m, n)),
                 ("used", torch.uint8, (k, m, n))]
        if steve:
            views += [("steve", torch.float32, (m,)), ("steve_weight", torch.float32, (k, m)), ("steve_mean", torch.float32, (k, m)),
                      ("steve_var", torch.float32, (k, m)), ("steve_count", torch.int32, (k, m)), ("steve_fallback", torch.uint8, (m,))]
        out = {}
        for (name, dtype, shape), o in zip(views, off):
            nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            out[name] = buf[int(o):int(o) + nbytes].view(dtype).view(shape)
        return out

    def guided_plan(self, policy, reward, value, uncertainty, actuator, prev, prefix, advance, track, targets, offset, knots, phase, constraints,
                    score, params, obs, cp_obs, cp_act, init_mean, init_var, n, carry=None, carry_valid=None, seed=0, call=0, out=None,
                    want_best_return=False):
        """`cadm_guided_plan`: the loop of `rewarded_plan` with the registered policy net's proposals (`policy`: a `policy_params`
        describing the net of `set_policy_net`; None = none, and `rewarded_plan`'s launches) rolled through the model once and placed
        among every iteration's candidates, behind the kept elites and the mean candidate.  Arguments behind `policy` as
        `rewarded_plan`; the workspace is the slot of `cadm_guided_workspace_bytes`, cached apart from the others."""
        return self._nest_plan("guided_plan", (policy, reward, value, uncertainty, actuator, prev, prefix, advance, track, targets, offset,
                               knots, phase, constraints, score, params), obs, cp_obs, cp_act, init_mean, init_var, n, carry, carry_valid,
                               seed, call, out, want_best_return)

    # ------------------------------------------------------------------ terminal value from Q critics (opt-in; csrc/critic.hip)
    @staticmethod
    def critic_params(hidden_sizes=(), activation="relu", n_critics=2, reduce="min", weight=1.0):
        """`cadm_critic_params`: hidden_sizes / activation -- as `value_params` (every critic is D + A -> h_1 -> .. -> h_L -> 1); n_critics
        -- C in 1 .. `_lib.MAX_CRITICS`; reduce -- "min" or "mean" over the critics (or its CADM_CRITIC_* number); weight -- what the
        reduced Q is multiplied by before it is added to a return, finite (it carries a discount gamma^H -- not on an
        engine with `set_discount`: the library then multiplies gamma^H in).  Needs no GPU."""
        if isinstance(n_critics, bool) or not isinstance(n_critics, (int, np.integer)) or not 1 <= int(n_critics) <= _lib.MAX_CRITICS:
            raise ValueError("critic n_critics must be an int in 1 .. %d, got %r" % (_lib.MAX_CRITICS, n_critics))
        if isinstance(reduce, str) and reduce in _lib.CRITIC_REDUCES:
            red = _lib.CRITIC_REDUCES[reduce]
        elif not isinstance(reduce, (bool, str)) and isinstance(reduce, (int, np.integer)) and int(reduce) in _lib.CRITIC_REDUCES.values():
            red = int(reduce)
        else:
            raise ValueError("critic reduce must be %s, got %r" % (" or ".join(repr(k) for k in _lib.CRITIC_REDUCES), reduce))
        prm = _lib.CriticParams()
        HipEngine._net_params(prm, "critic", hidden_sizes, activation, weight)
        prm.n_critics, prm.reduce = int(n_critics), red
        return prm

    def set_critic_nets(self, params, nets=None, in_mean=None, in_std=None):
        """`cadm_set_critic_nets`: registers the C = params.n_critics critics that `params` (`critic_params`) describes -- `nets` a list
        of C nets, each as `value_weights` takes them with D + A inputs, the shared input statistics in_mean / in_std [D + A] over
        [state ; action] as `set_value_net` takes them.  The library packs copies of its own, so a second call replaces the critics
        without touching anything else.  params None: the critics are cleared."""
        who, K = "set_critic_nets", self.D + self.A
        if params is None:
            self._check(self.lib.cadm_set_critic_nets(self._ctx, None, None, None, None, None, self.stream), "cadm_" + who)
            self._critic_src, self._critic_n = None, 0
            return
        if isinstance(nets, torch.nn.Sequential) or nets is None:
            raise ValueError("%s: nets must be a list of %d nets" % (who, params.n_critics))
        nets = list(nets)
        if len(nets) != params.n_critics:
            raise ValueError("%s: %d nets given, %d critics declared" % (who, len(nets), params.n_critics))
        layers = [wb for c, net in enumerate(nets) for wb in HipEngine._net_layers(self, who, params, net, K, 1, critic=c)]
        mean, std = HipEngine._net_stats(self, who, K, in_mean, in_std, "in_mean", "in_std")
        self._critic_src = HipEngine._net_register(self, who, params, layers, mean, std)
        self._critic_n = int(params.n_critics)

    def critic_eval(self, states, actions=None, want_each=False, want_actions=False):
        """`cadm_critic_eval`: the reduced Q of states [..., D] -> [...] (device tensors) through the planner's kernel, at the registered
        policy net's action (actions None) or at actions [..., A].  want_each: also every critic's q [C, ...]; want_actions: also the
        action that was used [..., A].  Returns q, or the tuple (q[, each][, actions])."""
        states, flat = HipEngine._flat_rows(self, "critic_eval", states, self.D)
        R = int(flat.shape[0])
        aflat = None
        if actions is not None:
            actions = self._t(actions)
            if tuple(actions.shape) != tuple(states.shape[:-1]) + (self.A,):
                raise ValueError("critic_eval: actions %r, expected %r" % (tuple(actions.shape), tuple(states.shape[:-1]) + (self.A,)))
            aflat = actions.reshape(-1, self.A).contiguous()
        q = torch.empty((R,), dtype=torch.float32, device=self.device)
        C = getattr(self, "_critic_n", 0) if want_each else 0      # (0: no critics registered, and the library says so)
        each = torch.empty((C, R), dtype=torch.float32, device=self.device) if want_each else None
        act = torch.empty((R, self.A), dtype=torch.float32, device=self.device) if want_actions else None
        self._check(self.lib.cadm_critic_eval(self._ctx, ptr(flat), ptr(aflat), R, ptr(q), ptr(each), ptr(act), self.stream), "cadm_critic_eval")
        lead = tuple(states.shape[:-1])
        res = (q.reshape(lead),)
        if want_each:
            res += (each.reshape((C,) + lead),)
        if want_actions:
            res += (act.reshape(lead + (self.A,)),)
        return res[0] if len(res) == 1 else res

    def critic_returns(self, traj, rows, params, first=None, want_q=False, out=None):
        """`cadm_critic_returns` on device tensors: traj [H,m,n,p,D] (a rollout's `traj_out`), rows [m,n,p] -> rows + weight * reduce_c
        Q_c(s, pi(s)), s = traj[H-1], per row under `params` (`critic_params`, describing the registered critics).  first [m,n,p] int32
        (None: every row): `constrain_returns`' first_violation -- a row with first < H keeps its bits.  want_q: (rows_out, q [m,n,p]),
        q NaN where skipped.  out: where the new rows go (may be `rows` itself)."""
        traj, rows, first, out = HipEngine._returns_args(self, "critic_returns", traj, rows, first, out)
        H, m, n, p, D = traj.shape
        q = torch.empty((m, n, p), dtype=torch.float32, device=self.device) if want_q else None
        self._check(self.lib.cadm_critic_returns(self._ctx, ct.byref(params), ptr(traj), ptr(first), m, n, ptr(rows), ptr(out), ptr(q),
                                                 self.stream), "cadm_critic_returns")
        return (out, q) if want_q else out

    def critic_plan(self, critic, policy, reward, value, uncertainty, actuator, prev, prefix, advance, track, targets, offset, knots, phase,
                    constraints, score, params, obs, cp_obs, cp_act, init_mean, init_var, n, carry=None, carry_valid=None, seed=0, call=0,
                    out=None, want_best_return=False):
        """`cadm_critic_plan`: the loop of `guided_plan` with `critic.weight` times the registered critics' reduced Q of every particle's
        last state, at the registered policy net's action, added to the particle returns where the terminal value would be (`critic`: a
        `critic_params` describing the critics of `set_critic_nets`; None = none, and `guided_plan`'s launches).  `policy` may be None
        while a policy net is registered.  Arguments behind `critic` as `guided_plan`; the workspace is the slot of
        `cadm_critic_workspace_bytes`, cached apart from the others."""
        return self._nest_plan("critic_plan", (critic, policy, reward, value, uncertainty, actuator, prev, prefix, advance, track, targets,
                               offset, knots, phase, constraints, score, params), obs, cp_obs, cp_act, init_mean, init_var, n, carry,
                               carry_valid, seed, call, out, want_best_return)

    # ------------------------------------------------------------------ the actor's log-density (opt-in; csrc/policy_logp.hip)
    @staticmethod
    def policy_logp_params(weight=1.0, space="action"):
        """`cadm_policy_logp_params`: weight -- what the step sum of log pi(a_t | s_t) is multiplied by before it is added to a return
        (beta of return + beta * sum_t log pi), a finite number, no bool; space -- "action" (the squashed actor's density, with the tanh
        Jacobian) or "pre_squash" (the Gaussian's density of u = atanh(y), no Jacobian), or its CADM_LOGP_* number.  Needs no GPU."""
        prm = _lib.PolicyLogpParams()
        prm.space = HipEngine.policy_logp_space(space)
        if isinstance(weight, (bool, np.bool_)) or not isinstance(weight, (int, float, np.integer, np.floating)):
            raise ValueError("policy log-density weight must be a finite number, got %r" % (weight,))
        w = float(np.float32(weight))
        if not math.isfinite(w):
            raise ValueError("policy log-density weight must be a finite number, got %r" % (weight,))
        prm.weight = w
        return prm

    @staticmethod
    def policy_logp_space(space):
        """The CADM_LOGP_* number of space "action" | "pre_squash" (or of the number itself); anything else is a ValueError."""
        if isinstance(space, str) and space in _lib.LOGP_SPACES:
            return _lib.LOGP_SPACES[space]
        if not isinstance(space, (bool, str)) and isinstance(space, (int, np.integer)) and int(space) in _lib.LOGP_SPACES.values():
            return int(space)
        raise ValueError("policy log-density space must be %s, got %r" % (" or ".join(repr(k) for k in _lib.LOGP_SPACES), space))

    def policy_log_prob(self, states, actions, space="action"):
        """`cadm_policy_logp`: log pi(a | s) of states [..., D] and actions [..., A] -> [...] (device tensors) under the registered
        policy net and its Gaussian head, through the planner's kernel; NaN for a row with a non-finite value in its state or action."""
        sp = HipEngine.policy_logp_space(space)
        states, flat = HipEngine._flat_rows(self, "policy_log_prob", states, self.D)
        actions = self._t(actions)
        if tuple(actions.shape) != tuple(states.shape[:-1]) + (self.A,):
            raise ValueError("policy_log_prob: actions %r, expected %r" % (tuple(actions.shape), tuple(states.shape[:-1]) + (self.A,)))
        aflat = actions.reshape(-1, self.A).contiguous()
        R = int(flat.shape[0])
        logp = torch.empty((R,), dtype=torch.float32, device=self.device)
        self._check(self.lib.cadm_policy_logp(self._ctx, ptr(flat), ptr(aflat), R, sp, ptr(logp), self.stream), "cadm_policy_logp")
        return logp.reshape(tuple(states.shape[:-1]))

    def policy_logp_returns(self, traj, obs, actions, rows, params, first=None, want_steps=False, out=None):
        """`cadm_policy_logp_returns` on device tensors, `reward_returns`' twin: traj [H,m,n,p,D] (a rollout's `traj_out`), obs [m,D],
        actions [m,n,H,A] (what the rollout read), rows [m,n,p] -> rows + weight * S per row under `params` (`policy_logp_params`), S
        the sum of log pi(a_t | s_t) over the counted steps in ascending t.  first [m,n,p] int32 (None: every step counts):
        `constrain_returns`' first_violation -- the steps t <= first count.  want_steps: (rows_out, steps [H,m,n,p], S [m,n,p]), steps
        NaN where not counted; else the steps go to a cached workspace.  out: where the new rows go (may be `rows` itself)."""
        traj, rows, first, out = HipEngine._returns_args(self, "policy_logp_returns", traj, rows, first, out)
        H, m, n, p, D = traj.shape
        obs, actions = self._t(obs), self._t(actions)
        if tuple(obs.shape) != (m, D):
            raise ValueError("policy_logp_returns: obs %r, expected contiguous %r" % (tuple(obs.shape), (m, D)))
        if tuple(actions.shape) != (m, n, H, self.A):
            raise ValueError("policy_logp_returns: actions %r, expected contiguous %r" % (tuple(actions.shape), (m, n, H, self.A)))
        steps = S = ws = None
        if want_steps:
            steps = torch.empty((H, m, n, p), dtype=torch.float32, device=self.device)
            S = torch.empty((m, n, p), dtype=torch.float32, device=self.device)
        else:
            need = self.lib.cadm_policy_logp_workspace_bytes(self._ctx, m, n)
            ws = getattr(self, "_logp_ws", None)
            if ws is None or ws.numel() < need:
                ws = self._logp_ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=self.device)
        self._check(self.lib.cadm_policy_logp_returns(self._ctx, ct.byref(params), ptr(traj), ptr(obs), ptr(actions), ptr(first), m, n,
                                                      ptr(rows), ptr(out), ptr(steps), ptr(S), ptr(ws), self.stream), "cadm_policy_logp_returns")
        return (out, steps, S) if want_steps else out

    def anchored_plan(self, logp, critic, policy, reward, value, uncertainty, actuator, prev, prefix, advance, track, targets, offset, knots,
                      phase, constraints, score, params, obs, cp_obs, cp_act, init_mean, init_var, n, carry=None, carry_valid=None, seed=0,
                      call=0, out=None, want_best_return=False):
        """`cadm_anchored_plan`: the loop of `critic_plan` with `logp.weight` times the step sum of the registered actor's log-density
        log pi(a_t | s_t) added to the particle returns, behind the learned reward and in front of the terminal value / Q (`logp`: a
        `policy_logp_params`; None = none, and `critic_plan`'s launches).  `policy` may be None while a policy net and its head are
        registered.  Arguments behind `logp` as `critic_plan`; the workspace is the slot of `cadm_anchored_workspace_bytes`, cached
        apart from the others."""
        return self._nest_plan("anchored_plan", (logp, critic, policy, reward, value, uncertainty, actuator, prev, prefix, advance, track,
                               targets, offset, knots, phase, constraints, score, params), obs, cp_obs, cp_act, init_mean, init_var, n,
                               carry, carry_valid, seed, call, out, want_best_return)

    # ------------------------------------------------------------------ open-loop prediction error along the horizon
    def _horizon_outputs(self, F, D, E=None):
        z = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        E = self.E if E is None else E
        return dict(se=z((F, D), torch.float32), spread=z((F, D), torch.float32), se_member=z((E, F, D), torch.float32),
                    count=z((F,), torch.int32), diverged=z((F,), torch.int32))

    def horizon_error(self, traj, truth, mask, calls=None, E=None, truth_ld=None):
        """`cadm_horizon_error` on device tensors: traj [F,m,1,p,D] (or [F,m,p,D]), truth [m,F,D], mask [m,F] -> dict of device
        tensors se / spread [F,D], se_member [E,F,D] (SUMS over the valid, finite windows) and count / diverged [F] int32.
        `calls`: window counts (multiples of 64 but the last) to cut the windows into several stage-1 launches -- the result is the
        same bits (tests, tools).  `E`: the number of members the p particles split into (default: the engine's; the kernel reads no
        model).  `truth_ld`: floats between the truth rows of consecutive windows (default F * D); truth is then [m, truth_ld],
        a window's F * D values first."""
        return self._window_stats("horizon_error", traj, truth, mask, calls, E, truth_ld, False, lambda E, D: (2 + E) * D + 2, self._horizon_out)

    def _horizon_out(self, F, D, p, E):
        """(the dict of `horizon_error`, what its two exports take for it: the five pointers, in the dict's order)"""
        out = self._horizon_outputs(F, D, E)
        return out, [ptr(v) for v in out.values()]

    def _window_stats(self, who, traj, truth, mask, calls, E, truth_ld, split, floats, outputs):
        """What `horizon_error` and `calibration_stats` share: `cadm_<who>` over the windows, in one stage-1 launch or one per entry of
        `calls`.  split: the members must divide the particles (and the refusal names E); floats(E, D): the partial sums of one block at
        one step; outputs(F, D, p, E) -> (the result dict, the export's arguments for it)."""
        traj, truth, mask = self._t(traj), self._t(truth), self._t(mask)
        F, m, p, D = traj.shape[0], traj.shape[1], traj.shape[-2], traj.shape[-1]
        E = self.E if E is None else int(E)
        ld = F * D if truth_ld is None else int(truth_ld)
        if (tuple(truth.shape) != ((m, F, D) if truth_ld is None else (m, ld)) or tuple(mask.shape) != (m, F) or traj.numel() != F * m * p * D
                or E < 1 or split and p % E):
            raise ValueError("%s: traj %r, truth %r, mask %r%s do not agree"
                             % (who, tuple(traj.shape), tuple(truth.shape), tuple(mask.shape), ", E %d" % E if split else ""))
        blocks = (m + 63) // 64
        partials = torch.empty((blocks * F * floats(E, D),), dtype=torch.float32, device=self.device)
        out, outs = outputs(F, D, p, E)
        export, w0 = getattr(self.lib, "cadm_" + who), 0
        for n in (calls or [m]):
            # a launch reads its windows' [F, n, p, D] slice as one tensor
            part = traj if n == m else traj.reshape(F, m, p, D)[:, w0:w0 + n].contiguous()
            self._check(export(ptr(part), ptr(truth[w0:]), ld, ptr(mask[w0:]), n, F, p, E, D, w0, ptr(partials), blocks, *outs,
                               int(w0 + n >= m), self.stream), "cadm_" + who)
            w0 += n
        if w0 != m:
            raise ValueError("%s: calls %r do not add up to %d windows" % (who, calls, m))
        return out

    def eval_horizon(self, dev, N, F, chunk=4096, seed=0, call=0, eps=None):
        """`cadm_eval_horizon` on the device-resident windowed dataset `dev` (what `fit` uploads: obs / obs_next [N,F*D], act
        [N,F*A], cp_obs / cp_act [N,.], plus future_bool [N,F] float32) -> the dict of `horizon_error`.  eps: injected noise
        [F,N,1,p,D] (parity tests)."""
        return self._eval_windows("eval_horizon", "cadm_eval_workspace_bytes", self._horizon_out, dev, N, F, chunk, seed, call, eps)

    def _eval_windows(self, who, sizer, outputs, dev, N, F, chunk, seed, call, eps):
        """What `eval_horizon` and `eval_calibration` share: `cadm_<who>` over the dataset in chunks, on a workspace of `sizer` bytes;
        outputs: as `_window_stats` takes it."""
        if chunk <= 0 or chunk % 64:
            raise ValueError("%s: chunk must be a positive multiple of 64, got %r" % (who, chunk))
        eps = None if eps is None else self._t(eps)
        mc = min(int(chunk), (N + 63) // 64 * 64)
        self.ensure_rollout(_lib.NOISE_NONE if self.deterministic else _lib.NOISE_INJECT if eps is not None else _lib.NOISE_PHILOX, min(mc, N), 1)
        nbytes = getattr(self.lib, sizer)(self._ctx, int(N), int(F), int(chunk))
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=self.device)
        out, outs = outputs(F, self.D, self.p, self.E)
        g = lambda k: ptr(dev.get(k))
        self._check(getattr(self.lib, "cadm_" + who)(self._ctx, g("obs"), g("act"), g("obs_next"), g("cp_obs") if self.C > 0 else None,
                                                     g("cp_act") if self.C > 0 else None, g("future_bool"), int(N), int(F), int(chunk), seed,
                                                     call, ptr(eps), ptr(ws), *outs, self.stream), "cadm_" + who)
        return out

    # ------------------------------------------------------------------ calibration of the predictive distribution (csrc/calibration.hip)
    def _calibration_outputs(self, F, D, p, E):
        i = lambda *shape: torch.empty(shape, dtype=torch.int32, device=self.device)
        z = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)
        out = dict(rank_hist=i(F, D, p + 1), rank_hist_member=i(E, F, D, p // E + 1), ties=i(F, D), degenerate=i(F, D), crps=z(F, D), z2=z(F, D),
                   nll=z(F, D), count=i(F), diverged=i(F))
        c = _lib.CalibrationOut()
        for k, v in out.items():
            setattr(c, k, v.data_ptr())
        return out, c

    def calibration_stats(self, traj, truth, mask, calls=None, E=None, truth_ld=None):
        """`cadm_calibration_stats` on device tensors: the arguments of `horizon_error` -> dict of device tensors rank_hist [F,D,p+1],
        rank_hist_member [E,F,D,p/E+1], ties / degenerate [F,D], count / diverged [F] (int32 counts) and crps / z2 / nll [F,D] (float32
        SUMS over the counted windows; z2 and nll leave the degenerate ones out)."""
        return self._window_stats("calibration_stats", traj, truth, mask, calls, E, truth_ld, True, lambda E, D: 3 * D, self._calibration_out)

    def _calibration_out(self, F, D, p, E):
        """(the dict of `calibration_stats`, what its two exports take for it: the struct of its pointers)"""
        out, c = self._calibration_outputs(F, D, p, E)
        return out, [ct.byref(c)]

    def eval_calibration(self, dev, N, F, chunk=4096, seed=0, call=0, eps=None):
        """`cadm_eval_calibration` on the device-resident windowed dataset `dev` (see `eval_horizon`: the same arguments, rollouts
        and noise keys) -> the dict of `calibration_stats`."""
        return self._eval_windows("eval_calibration", "cadm_eval_calibration_workspace_bytes", self._calibration_out, dev, N, F, chunk, seed,
                                  call, eps)

    # ------------------------------------------------------------------ forecast of a plan (opt-in; csrc/forecast.hip)
    def _forecast_outputs(self, m, n, H, p, E, rollout_returns=False):
        D = self.D
        z = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)
        out = dict(mean=z(m, n, H, D), member_mean=z(E, m, n, H, D), var_total=z(m, n, H, D), var_epistemic=z(m, n, H, D),
                   var_aleatoric=z(m, n, H, D), lo=z(m, n, H, D), hi=z(m, n, H, D), reward_mean=z(m, n, H), reward_var=z(m, n, H),
                   reward_member=z(E, m, n, H), returns=z(m, n, p),
                   diverged_step=torch.empty((m, n), dtype=torch.int32, device=self.device))
        if rollout_returns:
            out["rollout_returns"] = z(m, n, p)
        c = _lib.ForecastOut()
        for k, v in out.items():
            setattr(c, k, v.data_ptr())
        return out, c

    def forecast_stats(self, traj, obs, actions, band_k=1, E=None):
        """`cadm_forecast_stats` on device tensors: traj [H,m,n,p,D] (a rollout's `traj_out`; H may be below the engine's horizon, p
        need not be the engine's), obs [m,D], actions [m,n,H,A] raw -> dict of device tensors: mean / var_total / var_epistemic /
        var_aleatoric / lo / hi [m,n,H,D], member_mean [E,m,n,H,D], reward_mean / reward_var [m,n,H], reward_member [E,m,n,H], returns
        [m,n,p], diverged_step [m,n] int32.  VARIANCES; lo / hi are the band_k-th smallest / largest particle value.  E: the number
        of members the p particles split into (default: the engine's)."""
        traj, obs, actions = self._t(traj), self._t(obs), self._t(actions)
        E = self.E if E is None else int(E)
        if traj.dim() != 5 or actions.dim() != 4 or obs.dim() != 2:
            raise ValueError("forecast_stats: traj %r, obs %r, actions %r: expected [H,m,n,p,D], [m,D], [m,n,H,A]"
                             % (tuple(traj.shape), tuple(obs.shape), tuple(actions.shape)))
        H, m, n, p, D = traj.shape
        if D != self.D or tuple(obs.shape) != (m, D) or tuple(actions.shape) != (m, n, H, self.A):
            raise ValueError("forecast_stats: traj %r, obs %r, actions %r do not agree (D=%d, A=%d)"
                             % (tuple(traj.shape), tuple(obs.shape), tuple(actions.shape), self.D, self.A))
        out, c = self._forecast_outputs(m, n, H, p, max(E, 1))
        self._check(self.lib.cadm_forecast_stats(self._ctx, ptr(traj), ptr(obs), ptr(actions), m, n, H, p, E, int(band_k), ct.byref(c),
                                                 self.stream), "cadm_forecast_stats")
        return out

    def plan_forecast(self, obs, cp_obs, cp_act, actions, band_k=1, eps=None, seed=0, call=0):
        """`cadm_plan_forecast`: the context encoder, one rollout of the n given action sequences per env (actions [m,n,H,A], raw;
        eps [H,m,n,p,D] injected noise, else device Philox keyed (seed, call) under the forecast's own iteration word) and the
        statistics of its trajectories -> the dict of `forecast_stats` plus rollout_returns [m,n,p], the rollout's own returns."""
        obs, actions = self._t(obs), self._t(actions)
        cp_obs = None if cp_obs is None or self.C == 0 else self._t(cp_obs)
        cp_act = None if cp_act is None or self.C == 0 else self._t(cp_act)
        eps = None if eps is None else self._t(eps)
        if actions.dim() != 4 or obs.dim() != 2 or tuple(actions.shape) != (obs.shape[0], actions.shape[1], self.H, self.A) or obs.shape[1] != self.D:
            raise ValueError("plan_forecast: obs %r, actions %r: expected [m,%d] and [m,n,%d,%d]" % (tuple(obs.shape), tuple(actions.shape), self.D,
                                                                                                   self.H, self.A))
        m, n = actions.shape[0], actions.shape[1]
        if eps is not None and tuple(eps.shape) != (self.H, m, n, self.p, self.D):
            raise ValueError("plan_forecast: eps has shape %r, expected %r" % (tuple(eps.shape), (self.H, m, n, self.p, self.D)))
        if not self.discrete:      # (a discrete engine is refused by the library, with its message)
            self.ensure_rollout(_lib.NOISE_NONE if self.deterministic else _lib.NOISE_INJECT if eps is not None else _lib.NOISE_PHILOX, m, n)
        key = (m, n)
        if getattr(self, "_forecast_ws_key", None) != key:
            nbytes = self.lib.cadm_forecast_workspace_bytes(self._ctx, m, n)
            self._forecast_ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=self.device)
            self._forecast_ws_key = key
        out, c = self._forecast_outputs(m, n, self.H, self.p, self.E, rollout_returns=True)
        self._check(self.lib.cadm_plan_forecast(self._ctx, ptr(obs), ptr(cp_obs), ptr(cp_act), ptr(actions), ptr(eps), m, n, int(band_k),
                                                seed, call, ptr(self._forecast_ws), ct.byref(c), self.stream), "cadm_plan_forecast")
        return out

    # ------------------------------------------------------------------ training
    def train_configure(self, learning_rate, weight_decays, context_weight_decays, weight_decay_coeff, back_coeff,
                        max_batch, beta1=0.9, beta2=0.999, epsilon=1e-8):
        hp = TrainHParams()
        hp.learning_rate, hp.beta1, hp.beta2, hp.epsilon = learning_rate, beta1, beta2, epsilon
        hp.back_coeff, hp.weight_decay_coeff = back_coeff, weight_decay_coeff
        wd = list(weight_decays)
        for i in range(self.NH):
            hp.weight_decays[i] = wd[i]
        hp.weight_decays[self.NH] = wd[-1]            # both heads (core/utils.py:328,334)
        if self.C > 0:
            cwd = list(context_weight_decays)
            ncp = len(self.cp_hidden_sizes)
            for i in range(ncp):
                hp.context_weight_decays[i] = cwd[i]
            hp.context_weight_decays[ncp] = cwd[-1]   # cp_output (core/utils.py:610)
        self._check(self.lib.cadm_train_configure(self._ctx, ct.byref(hp), int(max_batch)), "cadm_train_configure")
        self._train_B = int(max_batch)

    def train_step(self, batch, train=True):
        """batch: dict of [E,B,.] tensors (obs, act, delta, obs_next, back_delta, cp_obs, cp_act; the
        last four may be None for the vanilla model).  Returns a device tensor [mse, back_mse, recon]."""
        B = batch["obs"].shape[1]
        g = lambda k: ptr(batch.get(k))
        losses = torch.empty((3,), dtype=torch.float32, device=self.device)
        self._check(self.lib.cadm_train_step(self._ctx, g("obs"), g("act"), g("delta"), g("obs_next"), g("back_delta"),
                                       g("cp_obs"), g("cp_act"), B, int(train), ptr(losses), self.stream),
              "cadm_train_step")
        return losses

    def train_step_rows(self, dev, F, row_w, row_f, idx, train=True):
        """One step on rows of the windowed device dataset `dev` (dict of [N, F*dim] / [N, dim] tensors): idx [E,B] int64
        row ids, row_w / row_f int64 (window, future offset) of every training row.  No gather is materialised."""
        B = idx.shape[1]
        if idx.stride(1) != 1:
            idx = idx.contiguous()
        g = lambda k: ptr(dev.get(k))
        losses = torch.empty((3,), dtype=torch.float32, device=self.device)
        self._check(self.lib.cadm_train_step_rows(self._ctx, g("obs"), g("act"), g("delta"), g("obs_next"), g("back_delta"),
                                            g("cp_obs"), g("cp_act"), int(F), ptr(row_w), ptr(row_f), ptr(idx), int(idx.stride(0)), B,
                                            int(train),
                                            ptr(losses), self.stream), "cadm_train_step_rows")
        return losses

    # ------------------------------------------------------------------ multi-GPU (RCCL communicator owned by the ctx)
    def dist_init(self, group=None):
        """Create the ctx's RCCL communicator over the ranks of a torch.distributed group (the group is only
        used to broadcast the 128-byte ncclUniqueId).  Afterwards cem_plan / rs_plan take the GLOBAL candidate
        count and run the sharded planner entirely on the stream, one ncclAllGather per CEM iteration."""
        import torch.distributed as dist
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        buf = ct.create_string_buffer(128)
        # rank 0 ALWAYS reaches the broadcast: a failure to draw the id (librccl missing, ...) travels as a status byte, so
        # the other ranks never wait in a broadcast that rank 0 skipped (mismatched collectives would hang)
        status, err = 1, None
        if rank == 0:
            try:
                self._check(self.lib.cadm_dist_unique_id(buf), "cadm_dist_unique_id")
            except _lib.CadmError as exc:
                status, err = 0, exc
        t = torch.tensor(list(buf.raw) + [status], dtype=torch.uint8, device=self.device if dist.get_backend(group) == "nccl" else "cpu")
        dist.broadcast(t, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        raw = t.cpu().tolist()
        if raw[128] != 1:
            raise err if err is not None else _lib.CadmError("cadm_dist_unique_id failed on rank 0 of the group")
        ident = bytes(raw[:128])
        with torch.cuda.device(self.device):
            self._check(self.lib.cadm_dist_init(self._ctx, ident, world, rank), "cadm_dist_init")
        nr, rk = self.dist_info()
        if nr != world or rk != rank:
            raise _lib.CadmError("RCCL communicator reports nranks=%d rank=%d, expected %d / %d" % (nr, rk, world, rank))
        self.dist_world, self.dist_rank = world, rank

    def dist_init_external(self, group=None):
        """The same sharded planner with the all-gather supplied by torch.distributed over `group`, whatever its backend (gloo, or nccl
        where the in-library communicator cannot be built): `cadm_cem_plan` / `cadm_rs_plan` run the loop of the RCCL path and call back
        into `planner.ExternalAllGather` once per CEM iteration.  Both pointers of a call lie inside this engine's planner workspace."""
        import torch.distributed as dist
        from . import planner as _planner
        world, rank = dist.get_world_size(group), dist.get_rank(group)

        def resolve(ptr_, nbytes):
            ws = self._ws
            off = int(ptr_) - ws.data_ptr()
            if ws is None or off < 0 or off + nbytes > ws.numel() or off % 4:
                raise _lib.CadmError("external all-gather: pointer outside the planner workspace")
            return ws[off:off + nbytes].view(torch.float32)
        ext = _planner.ExternalAllGather(group, resolve)
        self._check(self.lib.cadm_dist_init_external(self._ctx, world, rank, ct.cast(ext.cfunc, ct.c_void_p), None), "cadm_dist_init_external")
        self._ext = ext
        self.dist_world, self.dist_rank = world, rank

    def dist_destroy(self):
        self._check(self.lib.cadm_dist_destroy(self._ctx), "cadm_dist_destroy")
        self.dist_world, self.dist_rank = 1, 0
        self._ext = None

    def dist_info(self):
        """(nranks, rank) as RCCL itself reports them for the ctx's communicator (ncclCommCount / ncclCommUserRank)."""
        n, r = ct.c_int(0), ct.c_int(0)
        self._check(self.lib.cadm_dist_info(self._ctx, ct.byref(n), ct.byref(r)), "cadm_dist_info")
        return int(n.value), int(r.value)

    # ------------------------------------------------------------------ in-library kernel timing
    def profile_enable(self, on=True):
        self._check(self.lib.cadm_profile_enable(self._ctx, int(on)), "cadm_profile_enable")

    def profile_read(self):
        """-> (total milliseconds, launches) of the rollout kernel since the last read."""
        ms, cnt = ct.c_float(0.0), ct.c_int(0)
        self._check(self.lib.cadm_profile_read(self._ctx, ct.byref(ms), ct.byref(cnt)), "cadm_profile_read")
        return float(ms.value), int(cnt.value)

    # ------------------------------------------------------------------ developer hooks (libcadm_hip_dev.so only)
    def dev_set_rollout(self, kind="xdl", row_tiles=0):
        """Select the fp32-MFMA comparison kernel ("f32") / force a flavour of the production kernel on THIS engine (row_tiles: 0 = the
        launcher's plan, 1 / 2 = cooperative kernel with one / two row tiles per workgroup, 3 / 4 = wave-tile kernel with 8 / 4 tiles).
        Exists only when the engine was built on the developer library (HipEngine(..., lib=_lib.load_dev()))."""
        if not hasattr(self.lib, "cadm_dev_set_rollout"):
            raise _lib.CadmError("dev_set_rollout needs the developer library (HipEngine(..., lib=_lib.load_dev()))")
        self._check(self.lib.cadm_dev_set_rollout(self._ctx, {"xdl": _lib.DEV_ROLLOUT_XDL, "f32": _lib.DEV_ROLLOUT_F32}[kind],
                                                  int(row_tiles)), "cadm_dev_set_rollout")

    def dev_read_adam_moment(self, net, name, second=False):
        """Adam's first (second=False) / second moment of one trained tensor, shaped like the tensor.  With beta1 = 0 the first
        moment after ONE training step is that step's gradient exactly (m = 0 m + 1 g): how the tests read dL/dW, dL/db element
        by element.  Developer library only."""
        if not hasattr(self.lib, "cadm_dev_read_adam_moment"):
            raise _lib.CadmError("dev_read_adam_moment needs the developer library (HipEngine(..., lib=_lib.load_dev()))")
        nid = {"ff_model": _lib.NET_FF, "backward_model": _lib.NET_BACK, "context_model": _lib.NET_CTX}[net]
        if name in ("max_logvar", "min_logvar"):
            layer, is_bias = (-1 if name == "max_logvar" else -2), 0
        else:
            base, kind = name.rsplit("_", 1)
            if net == "context_model":
                layers = ["cp_hidden_%d" % i for i in range(len(self.cp_hidden_sizes))] + ["cp_output"]
            else:
                layers = ["hidden_%d" % i for i in range(self.NH)] + ["output_mu", "output_logvar"]
            layer, is_bias = layers.index(base), int(kind == "bias")
        out = torch.empty_like(self.nets[net][name])
        self._check(self.lib.cadm_dev_read_adam_moment(self._ctx, nid, layer, is_bias, int(second), ptr(out), out.numel(), self.stream),
                    "cadm_dev_read_adam_moment")
        return out

    def profile_read_collective(self):
        """-> (total milliseconds, calls) of the in-library ncclAllGather since the last read (sharded planner)."""
        ms, cnt = ct.c_float(0.0), ct.c_int(0)
        self._check(self.lib.cadm_profile_read_collective(self._ctx, ct.byref(ms), ct.byref(cnt)), "cadm_profile_read_collective")
        return float(ms.value), int(cnt.value)

    def predict_heads(self, obs, act, cp_obs=None, cp_act=None):
        """[E,B,.] inputs -> (mu [E,B,D] normalised, logvar [E,B,D] clamped or None)."""
        obs, act = self._t(obs), self._t(act)
        cp_obs = None if cp_obs is None else self._t(cp_obs)
        cp_act = None if cp_act is None else self._t(cp_act)
        B = obs.shape[1]
        mu = torch.empty((self.E, B, self.D), dtype=torch.float32, device=self.device)
        lv = None if self.deterministic else torch.empty_like(mu)
        self._check(self.lib.cadm_predict(self._ctx, ptr(obs), ptr(act), ptr(cp_obs), ptr(cp_act), B, ptr(mu), ptr(lv), self.stream),
              "cadm_predict")
        return mu, lv

    def train_reset(self):
        self._check(self.lib.cadm_train_reset(self._ctx, self.stream), "cadm_train_reset")


def C_void_p():
    return ct.c_void_p()
