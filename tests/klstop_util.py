"""Shared pieces of the KL-stop tests (tests/test_klstop_gpu.py): three learners over one
128-sample rollout (T 8 x E 16) at the C ABI, one per kernel variant of the control step --

    H  64, S  60, B 32, nmb 4, epochs 3   the 4-wave row kernel             12 steps
    H 256, S 120, B 64, nmb 2, epochs 4   the 8-wave row kernel, tile image   8 steps
    H 128, S 260, B 16, nmb 8, epochs 2   the chunked (wide) row kernels     16 steps

(16 slots, period 4).  old_logp is the start policy's own log-probability of the stored actions
(hwy_ppo_act), so a step's KL starts near 0 and grows with the steps at lr 3e-3: limits that trip
in mid-update exist.  Metrics rows start at a sentinel no kernel writes."""

import ctypes
import functools

import torch

DEV = torch.device("cuda", 0)
N_SAMPLES = 128
LEARNERS = [(64, 60, 32, 4, 3), (256, 120, 64, 2, 4), (128, 260, 16, 8, 2)]
MAX_STEPS, PERIOD = 16, 4
SENTINEL = -777.0
LR = 3e-3


def lib():
    from hwy.ppo_native import _bind, _bind_group
    from hwy.ppo_native import lib as _lib

    return _bind_group(_bind(_lib()))


def stream():
    from hwy.native import stream_ptr

    return stream_ptr()


@functools.lru_cache(maxsize=None)
def start(H, S):
    """Seeded weights and a rollout the start policy itself sampled (shared, never written)."""
    from hwy.ppo_native import PpoActArgs, PpoDims, param_layout

    _, numel = param_layout(S, H)
    g = torch.Generator(device=DEV).manual_seed(1000 * H + S)
    r = lambda *shape: torch.randn(*shape, device=DEV, generator=g)  # noqa: E731
    st = {"flat": r(numel) * 0.05, "states": r(N_SAMPLES, S), "adv": r(N_SAMPLES),
          "ret": r(N_SAMPLES), "perm": torch.randperm(N_SAMPLES, device=DEV, generator=g)}
    noise = r(N_SAMPLES, 2)
    st["pre"] = torch.zeros(N_SAMPLES, 2, device=DEV)
    st["old_lp"] = torch.zeros(N_SAMPLES, device=DEV)
    action, value = torch.zeros(N_SAMPLES, 2, device=DEV), torch.zeros(N_SAMPLES, device=DEV)
    a = PpoActArgs()
    a.dims = PpoDims(N_SAMPLES, S, H, 2)
    a.states, a.params, a.noise = st["states"].data_ptr(), st["flat"].data_ptr(), noise.data_ptr()
    a.action, a.pre_tanh = action.data_ptr(), st["pre"].data_ptr()
    a.logp, a.value, a.tiles = st["old_lp"].data_ptr(), value.data_ptr(), None
    assert lib().hwy_ppo_act(ctypes.byref(a), stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(st["old_lp"]).all())
    return st


class Learner:
    """One learner's own buffers (a fresh copy of the seeded start; Adam state zero)."""

    def __init__(self, H, S, B, nmb, epochs, lr=LR):
        from hwy.ppo_native import PpoDims

        L = lib()
        st = start(H, S)
        assert nmb * B <= N_SAMPLES
        self.st, self.B, self.nmb, self.epochs, self.steps = st, B, nmb, epochs, nmb * epochs
        self.lr = lr
        self.dims = PpoDims(B, S, H, 2)
        n = st["flat"].numel()
        self.flat = st["flat"].clone()
        self.grads = torch.zeros(n, device=DEV)
        self.m = torch.zeros(n, device=DEV)
        self.v = torch.zeros(n, device=DEV)
        self.counters = torch.zeros(2, dtype=torch.int32, device=DEV)
        self.metrics = torch.full((self.steps, 6), SENTINEL, device=DEV)
        ws = L.hwy_ppo_workspace_bytes(ctypes.byref(self.dims))
        self.tile_off = int(L.hwy_ppo_tile_image_offset(ctypes.byref(self.dims)))
        assert ws > 0 and 0 <= self.tile_off < ws
        self.workspace = torch.zeros(int(ws), dtype=torch.uint8, device=DEV)
        self.sync()

    def sync(self):
        a0 = self.args(0)
        assert lib().hwy_ppo_sync_params(ctypes.byref(a0), stream()) == 0

    def reset(self):
        """Back to the seeded start, in place (graphs and tables keep pointing here)."""
        self.flat.copy_(self.st["flat"])
        for t in (self.grads, self.m, self.v, self.counters, self.workspace):
            t.zero_()
        self.metrics.fill_(SENTINEL)
        self.sync()

    def args(self, i):
        from hwy.ppo_native import PpoArgs

        st, a = self.st, PpoArgs()
        a.dims = self.dims
        a.states, a.pre_tanh, a.old_logp = (st["states"].data_ptr(), st["pre"].data_ptr(),
                                            st["old_lp"].data_ptr())
        a.adv, a.ret = st["adv"].data_ptr(), st["ret"].data_ptr()
        a.idx = st["perm"].data_ptr() + i * self.B * 8
        a.params, a.grads = self.flat.data_ptr(), self.grads.data_ptr()
        a.adam_m, a.adam_v = self.m.data_ptr(), self.v.data_ptr()
        a.counters, a.metrics = self.counters.data_ptr(), self.metrics.data_ptr()
        a.workspace = self.workspace.data_ptr()
        a.eps_clip, a.value_coef, a.entropy_coef, a.max_grad_norm = 0.2, 0.5, 0.005, 0.5
        a.lr, a.beta1, a.beta2, a.adam_eps = self.lr, 0.9, 0.999, 1e-8
        a.grads_modified = 0
        return a

    @property
    def tile_image(self):
        """The weight tile image: the workspace's last sub-buffer."""
        return self.workspace[self.tile_off:]

    def state(self):
        """What a discarded step must leave alone (the gradient and the row kernels' scratch in
        the workspace are the step's own and are not part of it)."""
        return {"params": self.flat, "adam_m": self.m, "adam_v": self.v,
                "tile_image": self.tile_image}

    def solo_steps(self, k):
        """k steps alone: hwy_ppo_forward_backward + hwy_ppo_optimizer in update order."""
        L = lib()
        for s in range(k):
            a = self.args(s % self.nmb)
            assert L.hwy_ppo_forward_backward(ctypes.byref(a), stream()) == 0
            assert L.hwy_ppo_optimizer(ctypes.byref(a), stream()) == 0
        torch.cuda.synchronize()
        return self


class Sched:
    """Learners with one prepared schedule table and, with `limits`, a control block:
    limits[g] = None (kl_on 0) or the learner's kl_limit."""

    def __init__(self, learners, limits=None, lrs=None):
        from hwy.ppo_native import PpoArgs, PpoDims, PpoSchedPlan

        L = self.L = lib()
        G = self.G = len(learners)
        self.ls = [Learner(*l, **({} if lrs is None else {"lr": lrs[g]}))
                   for g, l in enumerate(learners)]
        dims = (PpoDims * G)(*[l.dims for l in self.ls])
        self.nmb = (ctypes.c_int32 * G)(*[l.nmb for l in self.ls])
        self.epochs = (ctypes.c_int32 * G)(*[l.epochs for l in self.ls])
        nb = L.hwy_ppo_sched_table_bytes(dims, self.nmb, G)
        assert nb > 0
        self.arr = (PpoArgs * G)()
        for g, l in enumerate(self.ls):
            a = l.args(0)
            ctypes.memmove(ctypes.byref(self.arr[g]), ctypes.byref(a), ctypes.sizeof(PpoArgs))
        self.table = torch.empty(int(nb), dtype=torch.uint8, device=DEV)
        self.plan = PpoSchedPlan()
        assert L.hwy_ppo_sched_prepare(self.arr, self.nmb, self.epochs, G, self.table.data_ptr(),
                                       ctypes.byref(self.plan), stream()) == 0
        self.ctl = self.stopped_at = None
        if limits is not None:
            self.set_limits(limits)

    def set_limits(self, limits):
        L, G = self.L, self.G
        lim = (ctypes.c_float * G)(*[0.0 if k is None else float(k) for k in limits])
        on = (ctypes.c_int32 * G)(*[int(k is not None) for k in limits])
        nb = int(L.hwy_ppo_sched_ctl_bytes(G))
        off = int(L.hwy_ppo_sched_ctl_stopped_offset(G))
        assert nb > 0 and nb % 256 == 0 and 0 < off and off + 4 * G <= nb
        self.ctl = torch.zeros(nb, dtype=torch.uint8, device=DEV)
        assert L.hwy_ppo_sched_ctl_prepare(ctypes.byref(self.plan), lim, on, self.ctl.data_ptr(),
                                           stream()) == 0
        self.stopped_at = self.ctl[off:off + 4 * G].view(torch.int32)

    def begin(self, st=None):
        st = stream() if st is None else st
        if self.ctl is None:
            return self.L.hwy_ppo_sched_begin(ctypes.byref(self.plan), self.table.data_ptr(), st)
        return self.L.hwy_ppo_sched_ctl_begin(ctypes.byref(self.plan), self.table.data_ptr(),
                                              self.ctl.data_ptr(), st)

    def step(self, slot, st=None):
        st = stream() if st is None else st
        if self.ctl is None:
            return self.L.hwy_ppo_sched_step(ctypes.byref(self.plan), self.table.data_ptr(), slot,
                                             st)
        return self.L.hwy_ppo_sched_ctl_step(ctypes.byref(self.plan), self.table.data_ptr(),
                                             self.ctl.data_ptr(), slot, st)

    def advance(self, slots, st=None):
        return self.L.hwy_ppo_sched_advance(ctypes.byref(self.plan), self.table.data_ptr(), slots,
                                            stream() if st is None else st)

    def set_lr(self, lr_dev):
        return self.L.hwy_ppo_sched_set_lr(ctypes.byref(self.plan), self.table.data_ptr(),
                                           lr_dev.data_ptr(), stream())

    def run_eager(self):
        assert self.begin() == 0
        for s in range(self.plan.max_steps):
            assert self.step(s) == 0
        torch.cuda.synchronize()
        return self

    def run_graph(self, P):
        """A captured graph of P slots plus the advance, replayed over the whole update."""
        from utils.graphs import capture

        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with capture(graph, stream=side):
                for s in range(P):
                    assert self.step(s) == 0
                assert self.advance(P) == 0
        torch.cuda.current_stream().wait_stream(side)
        assert self.begin() == 0
        for _ in range(-(-self.plan.max_steps // P)):
            graph.replay()
        torch.cuda.synchronize()
        return self

    def snapshot(self):
        return [{**{k: v.clone() for k, v in l.state().items()}, "metrics": l.metrics.clone(),
                 "counters": l.counters.clone()} for l in self.ls]


def first_trip(kls, limit):
    """The first step whose float32 KL is not <= limit (the rule of the control step), or None."""
    for j, k in enumerate(kls):
        if not (k <= limit):
            return j
    return None


def mid_update_limit(kls):
    """A float32 limit strictly between two stored KLs that trips in mid-update: the step j
    nearest the middle at which the KL sets a new maximum, and the midpoint of that maximum and
    the previous one.  Returns (limit, j)."""
    import numpy as np

    k = np.asarray(kls, np.float32)
    assert np.isfinite(k).all()
    records = [j for j in range(1, len(k) - 1) if k[j] > k[:j].max()]
    assert records, f"no step of {k.tolist()} sets a new KL maximum in mid-update"
    j = min(records, key=lambda j: abs(j - len(k) // 2))
    lo, hi = np.float32(k[:j].max()), np.float32(k[j])
    limit = np.float32((np.float64(lo) + np.float64(hi)) / 2)
    assert lo < limit < hi, (lo, limit, hi)
    assert first_trip(k.tolist(), float(limit)) == j
    return float(limit), j
