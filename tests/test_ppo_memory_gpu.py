"""The memory contract of the PPO ABI (include/hwy_ppo.h): every pointer of hwy_ppo_args /
hwy_ppo_act_args -- counters, metrics and the workspace included -- sits in one guarded arena
(guard_util.Arena: 64 rows of the buffer's own pitch and 256 words of canary on either side), the
workspace is exactly hwy_ppo_workspace_bytes long and filled with poison before
hwy_ppo_sync_params, the rollout sources have more rows than the minibatch, and every call must
(1) leave every guard word intact, (2) leave every input bit-identical, (3) leave outputs it was
not asked for alone, and (4) produce, bit for bit, what the same calls produce on separate
zero-initialised allocations (the conditions FusedPPO runs them under): grads, the metrics rows,
params, adam_m, adam_v, counters and the weight tile image.  There is no tolerance anywhere.

Poison: all-ones bytes (a NaN) and 0x7F7FFFFF (FLT_MAX, because x > 0 ? x : 0, fminf and fmaxf
swallow a NaN).  Every region of the workspace is a float array (struct Work in
csrc/ppo_kernels.hip: carve() hands out 17 float* sub-buffers and nothing else, restated as
ppo_ref_util.workspace_sizes), so no poison value can become an address or an index.

The kernels use no atomics; test_baseline_is_deterministic runs every baseline twice.

Shapes: ppo_ref_util.MEMORY_FUSED / MEMORY_GENERAL / memory_large / memory_act; each case asserts
from the device's own CU count that it lands on the paths it is there for
(test_ppo_memory_inputs.py asserts the same for the full chip without a GPU).  Sequences:
  a  sync_params, then forward_backward + optimizer on three minibatches (max_grad_norm 1e6,
     1e-3, 0.5: one unclipped, one clipped step)
  b  a, with every workspace byte outside the tile image poisoned again between steps: the image
     is the only state the workspace carries from one step to the next
  c  grads_modified = 1: the gradient is rewritten (and the workspace outside the image poisoned)
     between forward_backward and optimizer, which takes the norm from ppo_sumsq
Acting (d): hwy_ppo_act with and without a tile image, noise given and NULL;
hwy_ppo_value_masked with action / pre_tanh / logp non-NULL (they keep their fill) and NULL.
Grouped: hwy_ppo_group_step, hwy_ppo_mixed_step, hwy_ppo_sched_step, hwy_ppo_sched_ctl_step and
the grouped / mixed acting calls with three learners in ONE arena, tables and control block
exactly *_bytes long; each learner equals its solo baseline."""

import ctypes
import functools

import pytest
import torch

from guard_util import Arena, Plain
from hwy.native import lib, stream_ptr
from hwy.ppo_native import (PpoActArgs, PpoArgs, PpoDims, PpoGroupPlan, PpoMixedActPlan,
                            PpoMixedPlan, PpoSchedPlan, _bind, _bind_group, param_layout)
from ppo_ref_util import (FULL_CHIP, MEMORY_FUSED, MEMORY_GENERAL, act_kernel, fused_ok,
                          WORK_REGIONS, memory_act, memory_large, memory_paths, workspace_floats,
                          workspace_sizes)
from test_ppo_fused_gpu import _tile_image_floats

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

POISONS = {"nan": -1, "fltmax": 0x7F7FFFFF}  # int32 words: all-ones bytes, FLT_MAX
MGN = (1e6, 1e-3, 0.5)  # max_grad_norm of steps 0, 1, 2: unclipped, clipped, the default
ROLLOUT = ("states", "pre_tanh", "old_logp", "adv", "ret")
COMPARED = ("grads", "metrics", "params", "adam_m", "adam_v", "counters", "image")


def L():
    return _bind_group(_bind(lib()))


def _ws_bytes(B, S, H):
    return int(L().hwy_ppo_workspace_bytes(ctypes.byref(PpoDims(B, S, H, 2))))


@functools.lru_cache(None)
def chip():
    """(CUs, XCDs) the library sizes its partitions for.  The CU count is the device's; the XCD
    count, which torch does not report, is the divisor of it whose restated workspace sizes
    (ppo_ref_util.workspace_floats, pinned against the library in test_ppo_memory_inputs.py) are
    hwy_ppo_workspace_bytes at every shape of this module -- 8 on an unpartitioned MI355X."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    torch.cuda.current_device()  # the library reads the chip of the current device
    shapes = [c for c, _ in MEMORY_FUSED + MEMORY_GENERAL + memory_large(cus)]
    for xcds in (8, 4, 2, 1):
        if cus % xcds == 0 and all(4 * workspace_floats(S, H, B, cus, xcds) == _ws_bytes(B, S, H)
                                   for B, S, H in shapes):
            return cus, xcds
    raise AssertionError(f"the restated plan matches the library for no XCD count at {cus} CUs")


def _sync():
    torch.cuda.synchronize()


def call(mem, what, fn, inputs, unwritten=()):
    """One ABI call between arm() and check(): `inputs` are the buffers it may only read,
    `unwritten` the outputs it was not asked for; every other buffer is an output."""
    mem.set_role("output", *mem.names())
    mem.set_role("input", *inputs)
    mem.set_role("unwritten", *unwritten)
    mem.arm()
    rc = fn()
    _sync()
    assert rc == 0, (what, rc)
    mem.check(what)


# ------------------------------------------------------------------ inputs, drawn once per case
def _minibatch_idx(g, n, B, k):
    """B row indices out of n holding row 0 and row n - 1 (a single row alternates them)."""
    if B == 1:
        return torch.tensor([n - 1 if k % 2 == 0 else 0], dtype=torch.int64, device=DEV)
    mid = (torch.randperm(n - 2, device=DEV, generator=g) + 1)[:B - 2]
    ix = torch.cat([torch.tensor([0, n - 1], device=DEV), mid])
    return ix[torch.randperm(B, device=DEV, generator=g)].contiguous()


@functools.lru_cache(None)
def learner_data(B, S, H, nidx, seed=0):
    """Parameters (fan-in scaled), n = B + 9 rollout rows whose pre_tanh / old_logp / ret come
    from the policy itself in fp32 torch (finite ratios, some clipped), nidx minibatches' indices
    and as many replacement gradients (sequence c), as int32 words by buffer name."""
    g = torch.Generator(device=DEV).manual_seed(1000003 * seed + 7919 * B + 31 * S + H)
    offs, numel = param_layout(S, H, B)
    n = B + 9
    rnd = lambda *shape: torch.randn(*shape, device=DEV, generator=g)  # noqa: E731
    flat = torch.zeros(numel, device=DEV)
    fan = (S, 1, H, 1, H, 1, H, 1, 1, H, 1, H, 1)
    ends = offs[1:] + [numel]
    for i, (o, e) in enumerate(zip(offs, ends)):
        flat[o:e] = rnd(e - o) * (fan[i] ** -0.5 if fan[i] > 1 else 0.01)
    flat[offs[8]:offs[8] + 2] = torch.tensor([-0.4, 0.3], device=DEV)
    W = lambda i, r, c: flat[offs[i]:offs[i] + r * c].view(r, c)  # noqa: E731
    b = lambda i, r: flat[offs[i]:offs[i] + r]  # noqa: E731
    s = rnd(n, S)
    h = torch.relu(torch.relu(s @ W(0, H, S).T + b(1, H)) @ W(2, H, H).T + b(3, H))
    mean = torch.relu(h @ W(4, H, H).T + b(5, H)) @ W(6, 2, H).T + b(7, 2)
    v = (torch.relu(h @ W(9, H, H).T + b(10, H)) @ W(11, 1, H).T + b(12, 1)).squeeze(-1)
    std = flat[offs[8]:offs[8] + 2].exp()
    z = mean + std * rnd(n, 2).clamp(-2, 2)
    lp = (torch.distributions.Normal(mean, std).log_prob(z)
          - torch.log1p(-torch.tanh(z) ** 2 + 1e-6)).sum(-1)
    d = {"params": flat, "states": s, "pre_tanh": z, "old_logp": lp + 0.05 * rnd(n),
         "adv": rnd(n), "ret": v + rnd(n)}
    for k in range(nidx):
        d[f"idx{k}"] = _minibatch_idx(g, n, B, k)
        d[f"regrad{k}"] = rnd(numel) * 0.01
    for t in d.values():
        assert t.dtype == torch.int64 or bool(torch.isfinite(t).all())
    return {k: t.contiguous().view(-1).view(torch.int32).clone() for k, t in d.items()}


class Learner:
    """One learner's buffers under `tag` in a shared Arena / Plain.  split_idx: one guarded
    buffer per minibatch's indices (the solo calls read exactly B of them); otherwise the whole
    permutation is one buffer, as hwy_ppo_sched_prepare wants it."""

    def __init__(self, mem, B, S, H, nidx, rows, tag="", split_idx=True, seed=0, lr=3e-4):
        self.mem, self.B, self.S, self.H, self.nidx, self.tag = mem, B, S, H, nidx, tag
        self.rows, self.split_idx, self.seed, self.lr = rows, split_idx, seed, lr
        self.n = B + 9
        self.dims = PpoDims(B, S, H, 2)
        _, self.numel = param_layout(S, H, B)
        self.ws_words = _ws_bytes(B, S, H) // 4
        assert self.ws_words > 0
        off = int(L().hwy_ppo_tile_image_offset(ctypes.byref(self.dims)))
        self.img = None
        if off >= 0:
            self.img = (off // 4, _tile_image_floats(S, H))
            assert sum(self.img) == self.ws_words  # the image is the workspace's last region
        assert (off >= 0) == fused_ok(S, H)
        n = self.n
        for name, words, pitch in (("states", n * S, S), ("pre_tanh", n * 2, 2), ("old_logp", n, 1),
                                   ("adv", n, 1), ("ret", n, 1)):
            mem.add(tag + name, words, pitch)
        if split_idx:
            for k in range(nidx):
                mem.add(f"{tag}idx{k}", 2 * B, 2)
        else:
            mem.add(tag + "idx", 2 * B * nidx, 2)
        for name in ("params", "grads", "adam_m", "adam_v"):
            mem.add(tag + name, self.numel, 1)
        mem.add(tag + "counters", 2, 1)
        mem.add(tag + "metrics", 6 * rows, 6)
        mem.add(tag + "workspace", self.ws_words, max(2 * H, S))

    def nm(self, *names):
        return [self.tag + x for x in names]

    def idx_names(self):
        return self.nm(*[f"idx{k}" for k in range(self.nidx)]) if self.split_idx else self.nm("idx")

    def readonly(self):
        """What every step call may only read: the rollout sources and the indices."""
        return self.nm(*ROLLOUT) + self.idx_names()

    def state_names(self):
        return self.nm("params", "grads", "adam_m", "adam_v", "counters", "metrics", "workspace")

    def w(self, name):
        return self.mem.words(self.tag + name)

    def load(self, poison):
        """After mem.build(): the drawn inputs; with `poison` the whole workspace and the
        metrics rows hold it (a Plain memory keeps its zeros)."""
        d = learner_data(self.B, self.S, self.H, self.nidx, self.seed)
        for name in ("params",) + ROLLOUT:
            self.w(name).copy_(d[name])
        for k in range(self.nidx):
            if self.split_idx:
                self.w(f"idx{k}").copy_(d[f"idx{k}"])
            else:
                self.w("idx")[2 * self.B * k:2 * self.B * (k + 1)].copy_(d[f"idx{k}"])
        self.regrad = [d[f"regrad{k}"] for k in range(self.nidx)]
        if poison is not None:
            self.w("workspace").fill_(poison)
            self.w("metrics").fill_(poison)

    def poison_scratch(self, poison):
        """Every workspace byte outside the tile image."""
        if poison is not None:
            self.w("workspace")[:self.img[0] if self.img else self.ws_words].fill_(poison)

    def check_slack(self, poison, what):
        """The guard words a single workspace pointer leaves room for: carve() rounds each of
        its 17 regions up to 64 floats, and the words so added belong to no region, so on a
        poisoned workspace they still hold the poison after any call -- unless a region's ragged
        tile bled past its end.  (A bleed that ends inside the next region is rewritten by that
        region's own stores and cannot be seen from outside.)"""
        if poison is None:
            return
        w, o = self.w("workspace"), 0
        for name, n in zip(WORK_REGIONS, workspace_sizes(self.S, self.H, self.B, *chip())):
            end = -(-n // 64) * 64
            bad = w[o + n:o + end] != poison
            assert not bool(bad.any()), (
                f"{what}: the rounding slack after workspace region '{name}' ({n} floats) was"
                f" written, first at float {n + int(bad.nonzero()[0]) if bool(bad.any()) else -1}"
                f" of the region")
            o += end
        assert o == self.ws_words

    def poison_grads(self, poison):
        """forward_backward writes the whole flat gradient: what it held before cannot matter."""
        if poison is not None:
            self.w("grads").fill_(poison)

    def args(self, k=0, mgn=0.5, grads_modified=0):
        a, p = PpoArgs(), lambda name: self.mem.ptr(self.tag + name)  # noqa: E731
        a.dims = self.dims
        a.states, a.pre_tanh, a.old_logp, a.adv, a.ret = (p(x) for x in ROLLOUT)
        a.idx = p(f"idx{k}") if self.split_idx else p("idx") + 8 * self.B * k
        a.params, a.grads, a.adam_m, a.adam_v = (p(x) for x in ("params", "grads", "adam_m", "adam_v"))
        a.counters, a.metrics, a.workspace = p("counters"), p("metrics"), p("workspace")
        a.eps_clip, a.value_coef, a.entropy_coef, a.max_grad_norm = 0.2, 0.5, 0.005, mgn
        a.lr, a.beta1, a.beta2, a.adam_eps = self.lr, 0.9, 0.999, 1e-8
        a.grads_modified = grads_modified
        return a

    def state(self, rows):
        """Clones of what a step leaves behind: the first `rows` metrics rows and the image."""
        out = {k: self.w(k).clone() for k in ("grads", "params", "adam_m", "adam_v", "counters")}
        out["metrics"] = self.w("metrics")[:6 * rows].clone()
        if self.img:
            out["image"] = self.w("workspace")[self.img[0]:sum(self.img)].clone()
        return out

    def image(self):
        return self.w("workspace")[self.img[0]:sum(self.img)] if self.img else None


def same(got, want, what, keys=COMPARED):
    for k in keys:
        if k in want:
            diff = got[k] != want[k]
            assert not bool(diff.any()), (
                f"{what}: {k} differs from the zero-workspace baseline in {int(diff.sum())} of "
                f"{diff.numel()} words, first at {int(diff.nonzero()[0])}")


# ------------------------------------------------------------------ solo sequences
def run_solo(mem, B, S, H, seq, poison, steps, tag="", nidx=None, mgns=MGN, seed=0, lr=3e-4,
             learner=None):
    """sync_params, then `steps` x (forward_backward, optimizer) on minibatch step % nidx; the
    states after sync_params and after every step."""
    nidx = nidx or steps
    own = learner is None
    ln = learner or Learner(mem, B, S, H, nidx, steps, tag, seed=seed, lr=lr)
    if own:
        mem.build()
        ln.load(poison)
    lib_ = L()
    where = f"{B}-{S}-{H} {seq}"
    every = ln.readonly() + ln.nm("params", "grads", "adam_m", "adam_v", "counters", "metrics")
    a0 = ln.args(0)
    call(mem, f"{where} sync_params", lambda: lib_.hwy_ppo_sync_params(ctypes.byref(a0), stream_ptr()),
         every)
    out = [ln.state(0)]
    for k in range(steps):
        if seq == "b" and k:
            ln.poison_scratch(poison)
        ln.poison_grads(poison)
        a = ln.args(k % nidx, mgns[k % len(mgns)], 1 if seq == "c" else 0)
        call(mem, f"{where} step {k} forward_backward",
             lambda: lib_.hwy_ppo_forward_backward(ctypes.byref(a), stream_ptr()),
             ln.readonly() + ln.nm("params", "adam_m", "adam_v"))
        ln.check_slack(poison, f"{where} step {k} forward_backward")
        if seq == "c":
            ln.w("grads").copy_(ln.regrad[k % nidx])
            ln.poison_scratch(poison)
        call(mem, f"{where} step {k} optimizer",
             lambda: lib_.hwy_ppo_optimizer(ctypes.byref(a), stream_ptr()),
             ln.readonly() + ln.nm("grads", "counters", "metrics"))
        ln.check_slack(poison, f"{where} step {k} optimizer")
        out.append(ln.state(k + 1))
    return out


@functools.lru_cache(None)
def baseline(B, S, H, seq, steps, nidx=None, mgns=MGN, seed=0, lr=3e-4):
    return run_solo(Plain(DEV), B, S, H, seq, None, steps, nidx=nidx, mgns=mgns, seed=seed, lr=lr)


# (B, S, H) or, for the shapes that depend on the chip's CU count, their path (resolved on the
# device by _shape, so that collecting the module touches no GPU); the tags; the steps run
STEP_CASES = ([(c, want, 3) for c, want in MEMORY_FUSED + MEMORY_GENERAL]
              + [("rows32", None, 1), ("rows64", None, 1)])  # one step above 8,000 rows
ACT_CASES = memory_act(FULL_CHIP[0])[:-1] + ("act_c32",)


def _shape(c):
    """A case's (B, S, H) and tags on this device."""
    cus = chip()[0]
    if c[0] in ("rows32", "rows64"):
        return memory_large(cus)[("rows32", "rows64").index(c[0])] + (c[2],)
    if c == "act_c32":
        return memory_act(cus)[-1]
    return c


_cid = lambda c: c[0] if isinstance(c[0], str) else "-".join(map(str, c[0]))  # noqa: E731


def _check_baseline(states, B, S, H, seq, steps):
    """The baseline is a real update: finite, every step moved the weights and the image, the
    metrics rows and counters are the steps', and steps 0 / 1 ran unclipped / clipped."""
    for k in range(1, steps + 1):
        st, prev = states[k], states[k - 1]
        for name in ("grads", "params", "adam_m", "adam_v", "metrics"):
            assert bool(torch.isfinite(st[name].view(torch.float32)).all()), (k, name)
        assert not torch.equal(st["params"], prev["params"]), k
        assert st["counters"].tolist() == [k, k], k
        if "image" in st:
            assert not torch.equal(st["image"], prev["image"]), k
        norm = float(st["grads"].view(torch.float32).double().norm())
        assert 0.0 < norm, k
        if k <= 2:
            assert (norm > MGN[k - 1]) == (k == 2), (k, norm)


@pytest.mark.parametrize("seq", ["a", "b", "c"])
@pytest.mark.parametrize("c", STEP_CASES, ids=_cid)
def test_baseline_is_deterministic(c, seq):
    """The same calls on fresh zero-initialised allocations twice: bit-identical (no atomics),
    which is what lets every other test of this module ask for bit equality."""
    (B, S, H), want, steps = _shape(c)
    got = memory_paths(S, H, B, *chip())
    assert want <= got, (want - got, got)
    first = baseline(B, S, H, seq, steps)
    _check_baseline(first, B, S, H, seq, steps)
    again = run_solo(Plain(DEV), B, S, H, seq, None, steps)
    for k, (x, y) in enumerate(zip(again, first)):
        same(x, y, f"{B}-{S}-{H} {seq} second baseline run, state {k}")


@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("seq", ["a", "b", "c"])
@pytest.mark.parametrize("c", STEP_CASES, ids=_cid)
def test_step_between_guards_on_a_poisoned_workspace(c, seq, poison):
    (B, S, H), want, steps = _shape(c)
    got = memory_paths(S, H, B, *chip())
    assert want <= got, (want - got, got)
    base = baseline(B, S, H, seq, steps)
    states = run_solo(Arena(DEV), B, S, H, seq, POISONS[poison], steps)
    for k, (x, y) in enumerate(zip(states, base)):
        same(x, y, f"{B}-{S}-{H} {seq} {poison} state {k} (0: after sync_params)")


# ------------------------------------------------------------------ acting
class Actor:
    """hwy_ppo_act_args in a shared memory: exactly B rows of every buffer."""

    OUT = ("action", "out_pre_tanh", "logp", "value")

    def __init__(self, mem, B, S, H, tag="", seed=0):
        self.mem, self.B, self.S, self.H, self.tag, self.seed = mem, B, S, H, tag, seed
        self.dims = PpoDims(B, S, H, 2)
        _, self.numel = param_layout(S, H, B)
        # the tile image depends on S and H only: a 16-row workspace carries it
        self.wdims = PpoDims(16, S, H, 2)
        self.ws_words = _ws_bytes(16, S, H) // 4
        self.img = (int(L().hwy_ppo_tile_image_offset(ctypes.byref(self.wdims))) // 4,
                    _tile_image_floats(S, H))
        assert sum(self.img) == self.ws_words
        for name, words, pitch in (("states", B * S, S), ("params", self.numel, 1), ("noise", 2 * B, 2),
                                   ("action", 2 * B, 2), ("out_pre_tanh", 2 * B, 2), ("logp", B, 1),
                                   ("value", B, 1), ("truncated", -(-B // 4), 1),
                                   ("truncated_u", -(-B // 4), 1), ("terminated", -(-B // 4), 1),
                                   ("workspace", self.ws_words, max(2 * H, S))):
            mem.add(tag + name, words, pitch)

    def nm(self, *names):
        return [self.tag + x for x in names]

    def w(self, name):
        return self.mem.words(self.tag + name)

    def load(self, poison):
        B, S = self.B, self.S
        g = torch.Generator(device=DEV).manual_seed(11 + self.seed)
        self.w("params").copy_(learner_data(B, S, self.H, 1, self.seed)["params"])
        self.w("states").copy_(torch.randn(B * S, device=DEV, generator=g).view(torch.int32))
        self.w("noise").copy_(torch.randn(2 * B, device=DEV, generator=g).clamp(-2, 2).view(torch.int32))
        tr = (torch.rand(B, device=DEV, generator=g) < 0.4)
        te = (torch.rand(B, device=DEV, generator=g) < 0.3)
        tr[16:32] = False  # a 16-row tile without a marked row returns before it reads a weight
        tr[0] = tr[B - 1] = True
        te[0] = te[B - 1] = False
        # truncated_u: the last (ragged) 16- and 32-row tile holds no marked row, so its zeros
        # come from the early store; with `truncated` its last row is marked
        tu = tr.clone()
        tu[(B - 1) // 32 * 32:] = False
        self.mem.u8(self.tag + "truncated")[:B].copy_(tr.to(torch.uint8))
        self.mem.u8(self.tag + "truncated_u")[:B].copy_(tu.to(torch.uint8))
        self.mem.u8(self.tag + "terminated")[:B].copy_(te.to(torch.uint8))
        self.marked = {True: tr & ~te, False: tu & ~te}
        if poison is not None:
            self.w("workspace").fill_(poison)

    def sync_args(self):
        a = PpoArgs()
        a.dims = self.wdims
        a.params, a.workspace = self.mem.ptr(self.tag + "params"), self.mem.ptr(self.tag + "workspace")
        return a

    def args(self, tiles, noise=True, outs=True):
        a, p = PpoActArgs(), lambda name: self.mem.ptr(self.tag + name)  # noqa: E731
        a.dims = self.dims
        a.states, a.params = p("states"), p("params")
        a.noise = p("noise") if noise else None
        if outs:
            a.action, a.pre_tanh, a.logp = p("action"), p("out_pre_tanh"), p("logp")
        a.value = p("value")
        a.tiles = p("workspace") + 4 * self.img[0] if tiles else None
        return a

    def inputs(self):
        return self.nm("states", "params", "noise", "truncated", "truncated_u", "terminated",
                       "workspace")

    def outputs(self):
        return {k: self.w(k).clone() for k in self.OUT}


ACT_VARIANTS = [(t, n) for t in (0, 1) for n in (True, False)]
# tile image, action / pre_tanh / logp given, last tile holding a marked row
VMASK_VARIANTS = [(t, o, m) for t in (0, 1) for o in (True, False) for m in (True, False)]


def run_act(mem, B, S, H, poison):
    """Every acting variant of one shape; {variant: outputs}."""
    ac = Actor(mem, B, S, H)
    mem.build()
    ac.load(poison)
    lib_, where, out = L(), f"act {B}-{S}-{H}", {}
    sa = ac.sync_args()
    call(mem, f"{where} sync_params", lambda: lib_.hwy_ppo_sync_params(ctypes.byref(sa), stream_ptr()),
         [n for n in ac.inputs() if n != ac.tag + "workspace"], ac.nm(*Actor.OUT))
    for tiles, noise in ACT_VARIANTS:
        a = ac.args(tiles, noise)
        for k in Actor.OUT:
            ac.w(k).fill_(0x7FC54321)
        call(mem, f"{where} hwy_ppo_act tiles={tiles} noise={noise}",
             lambda: lib_.hwy_ppo_act(ctypes.byref(a), stream_ptr()), ac.inputs())
        out["act", tiles, noise] = ac.outputs()
    term = mem.ptr(ac.tag + "terminated")
    for tiles, outs, last in VMASK_VARIANTS:
        a = ac.args(tiles, False, outs)
        trunc = mem.ptr(ac.tag + ("truncated" if last else "truncated_u"))
        ac.w("value").fill_(0x7FC54321)
        # non-NULL action / pre_tanh / logp are not written: "Nothing else is written"
        call(mem, f"{where} hwy_ppo_value_masked tiles={tiles} outs={outs} last tile marked={last}",
             lambda: lib_.hwy_ppo_value_masked(ctypes.byref(a), trunc, term, stream_ptr()),
             ac.inputs(), ac.nm("action", "out_pre_tanh", "logp"))
        out["vmask", tiles, outs, last] = {"value": ac.w("value").clone()}
    out["marked"] = ac.marked
    return out


@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("c", ACT_CASES, ids=lambda c: c if isinstance(c, str) else "-".join(map(str, c)))
def test_acting_between_guards(c, poison):
    cus = chip()[0]
    B, S, H = _shape(c)
    if c == ACT_CASES[-2]:
        assert act_kernel(S, H, B, 1, cus) == ("ppo_act_c", 16) and B % 16
    if c == ACT_CASES[-1]:
        assert act_kernel(S, H, B, 1, cus) == ("ppo_act_c", 32) and B % 32
    base = run_act(Plain(DEV), B, S, H, None)
    got = run_act(Arena(DEV), B, S, H, POISONS[poison])
    marked = base["marked"]
    for key, want in base.items():
        if key == "marked":
            continue
        same(got[key], want, f"act {B}-{S}-{H} {key}", keys=tuple(want))
        for name, t in want.items():
            assert bool(torch.isfinite(t.view(torch.float32)).all()), (key, name)
    # the baseline is the documented one: deterministic acting has log-prob 0 and z = mean;
    # a masked value is acting's bits on a marked row and exactly +0.0 on every other
    for tiles in (0, 1):
        det = base["act", tiles, False]
        assert not bool(det["logp"].any())
        assert torch.equal(det["value"], base["act", tiles, True]["value"])
        for _, outs, last in VMASK_VARIANTS[:4]:
            v, mk = base["vmask", tiles, outs, last]["value"], marked[last]
            assert torch.equal(v[mk], det["value"][mk]) and not bool(v[~mk].any())
            assert bool(mk[B - 1]) == last


# ------------------------------------------------------------------ grouped learners
def _solo_baselines(dims, steps, nidx, mgns=(0.5,), lrs=None):
    return [baseline(B, S, H, "a", st, nidx=ni, mgns=mgns, seed=g + 1,
                     lr=3e-4 if lrs is None else lrs[g])
            for g, ((B, S, H), st, ni) in enumerate(zip(dims, steps, nidx))]


def _group(mem, dims, steps, nidx, poison, split_idx, lrs=None):
    """G learners in one memory (tags l0_, l1_, ...), built, loaded and synced solo."""
    ls = [Learner(mem, B, S, H, ni, st, f"l{g}_", split_idx=split_idx, seed=g + 1,
                  lr=3e-4 if lrs is None else lrs[g])
          for g, ((B, S, H), st, ni) in enumerate(zip(dims, steps, nidx))]
    return ls


def _sync_all(mem, ls, extra_inputs=()):
    lib_ = L()
    for ln in ls:
        a = ln.args(0)
        others = [n for n in mem.names() if n != ln.tag + "workspace"]
        call(mem, f"{ln.tag} sync_params", lambda: lib_.hwy_ppo_sync_params(ctypes.byref(a), stream_ptr()),
             others)


def _args_array(ls, k):
    arr = (PpoArgs * len(ls))()
    for g, ln in enumerate(ls):
        a = ln.args(k)
        ctypes.memmove(ctypes.byref(arr[g]), ctypes.byref(a), ctypes.sizeof(PpoArgs))
    return arr


def _per_minibatch_group(kind, dims, poison):
    """hwy_ppo_group_step / hwy_ppo_mixed_step: three minibatches, one table per minibatch."""
    G, nmb = len(dims), 3
    lib_ = L()
    base = _solo_baselines(dims, [nmb] * G, [nmb] * G)
    mem = Arena(DEV)
    ls = _group(mem, dims, [nmb] * G, [nmb] * G, poison, True)
    dd = (PpoDims * G)(*[ln.dims for ln in ls])
    nb = int(lib_.hwy_ppo_group_table_bytes(ctypes.byref(dd[0]), G) if kind == "group"
             else lib_.hwy_ppo_mixed_table_bytes(dd, G))
    assert nb > 0 and nb % 4 == 0, nb
    tables = [mem.add(f"table{i}", nb // 4, 1) for i in range(nmb)]
    mem.build()
    for ln in ls:
        ln.load(poison)
    _sync_all(mem, ls)
    plans = []
    for i in range(nmb):
        arr = _args_array(ls, i)
        plan = PpoGroupPlan() if kind == "group" else PpoMixedPlan()
        prep = lib_.hwy_ppo_group_prepare if kind == "group" else lib_.hwy_ppo_mixed_prepare
        call(mem, f"{kind} prepare {i}",
             lambda: prep(arr, G, mem.ptr(tables[i]), ctypes.byref(plan), stream_ptr()),
             [n for n in mem.names() if n != tables[i]])
        plans.append(plan)
    step = lib_.hwy_ppo_group_step if kind == "group" else lib_.hwy_ppo_mixed_step
    for g, ln in enumerate(ls):
        same(ln.state(0), base[g][0], f"{kind} learner {g} after sync_params")
    for i in range(nmb):
        for ln in ls:
            ln.poison_scratch(poison)
            ln.poison_grads(poison)
        call(mem, f"{kind} step {i}",
             lambda: step(ctypes.byref(plans[i]), mem.ptr(tables[i]), stream_ptr()),
             sum((ln.readonly() for ln in ls), []) + tables)
        for g, ln in enumerate(ls):
            same(ln.state(i + 1), base[g][i + 1], f"{kind} learner {g} after step {i}")
            ln.check_slack(poison, f"{kind} learner {g} after step {i}")


GROUP_DIMS = ((40, 60, 128), (40, 120, 128), (40, 300, 128))    # same H, S 60 / 120 / 300
MIXED_DIMS = ((40, 60, 64), (40, 120, 256), (40, 200, 320))     # H 64 / 256 / 320
SCHED_DIMS = ((40, 60, 64), (24, 120, 256), (17, 200, 320))     # B differs as well
SCHED_NMB, SCHED_EPOCHS = (3, 2, 1), (1, 1, 2)                  # steps 3, 2, 2 of 3 slots


@pytest.mark.parametrize("poison", list(POISONS))
def test_group_step_learners_in_one_arena(poison):
    _per_minibatch_group("group", GROUP_DIMS, POISONS[poison])


@pytest.mark.parametrize("poison", list(POISONS))
def test_mixed_step_learners_in_one_arena(poison):
    _per_minibatch_group("mixed", MIXED_DIMS, POISONS[poison])


def _trip_slot(rows):
    """The slot at which a KL limit between two steps' KL trips, and that limit: the first
    step whose KL exceeds every earlier one's (rows: a solo baseline's metrics rows)."""
    kl = [float(r[5]) for r in rows]
    for t in range(1, len(kl)):
        if kl[t] > max(kl[:t]):
            return t, 0.5 * (max(kl[:t]) + kl[t])
    raise AssertionError(f"the KL of the tripping learner never rises: {kl}")


@pytest.mark.parametrize("ctl", [False, True], ids=["sched", "sched_ctl"])
@pytest.mark.parametrize("poison", list(POISONS))
def test_sched_update_learners_in_one_arena(poison, ctl):
    """One whole scheduled update (3 slots; learners 1 and 2 sit slot 2 out, untouched).  With
    the control block learner 0 trips: that step is dropped and from then on its params, moments
    and tile image do not change."""
    poison = POISONS[poison]
    G, dims = 3, SCHED_DIMS
    lib_ = L()
    steps = [n * e for n, e in zip(SCHED_NMB, SCHED_EPOCHS)]
    lrs = (1e-2, 3e-4, 3e-4) if ctl else None  # a learning rate at which learner 0's KL rises
    base = _solo_baselines(dims, steps, SCHED_NMB, lrs=lrs)
    mem = Arena(DEV)
    ls = _group(mem, dims, steps, SCHED_NMB, poison, False, lrs=lrs)
    dd = (PpoDims * G)(*[ln.dims for ln in ls])
    nmb = (ctypes.c_int32 * G)(*SCHED_NMB)
    epochs = (ctypes.c_int32 * G)(*SCHED_EPOCHS)
    nb = int(lib_.hwy_ppo_sched_table_bytes(dd, nmb, G))
    assert nb > 0 and nb % 4 == 0, nb
    mem.add("table", nb // 4, 1)
    trip = None
    if ctl:
        cb = int(lib_.hwy_ppo_sched_ctl_bytes(G))
        assert cb > 0 and cb % 4 == 0
        mem.add("ctl", cb // 4, 1)
        rows0 = base[0][-1]["metrics"].view(torch.float32).view(-1, 6).cpu()
        trip, limit = _trip_slot(rows0)
    mem.build()
    for ln in ls:
        ln.load(poison)
    _sync_all(mem, ls)
    arr, plan = _args_array(ls, 0), PpoSchedPlan()
    call(mem, "sched prepare",
         lambda: lib_.hwy_ppo_sched_prepare(arr, nmb, epochs, G, mem.ptr("table"), ctypes.byref(plan),
                                            stream_ptr()),
         [n for n in mem.names() if n != "table"])
    assert plan.max_steps == max(steps)
    everything = [n for n in mem.names() if n not in ("table", "ctl")]
    if ctl:
        lim = (ctypes.c_float * G)(limit, 0.0, 0.0)
        on = (ctypes.c_int32 * G)(1, 0, 0)
        call(mem, "ctl prepare",
             lambda: lib_.hwy_ppo_sched_ctl_prepare(ctypes.byref(plan), lim, on, mem.ptr("ctl"),
                                                    stream_ptr()), everything + ["table"])
        call(mem, "ctl begin",
             lambda: lib_.hwy_ppo_sched_ctl_begin(ctypes.byref(plan), mem.ptr("table"),
                                                  mem.ptr("ctl"), stream_ptr()), everything)
    else:
        call(mem, "sched begin",
             lambda: lib_.hwy_ppo_sched_begin(ctypes.byref(plan), mem.ptr("table"), stream_ptr()),
             everything)
    for s in range(plan.max_steps):
        tripped = ctl and s > trip
        active = [g for g in range(G) if s < steps[g] and not (g == 0 and tripped)]
        inputs = sum((ln.readonly() for ln in ls), []) + ["table"]
        for g, ln in enumerate(ls):
            if g in active:
                ln.poison_scratch(poison)
                ln.poison_grads(poison)
            elif g == 0 and tripped:
                inputs += ln.nm("params", "adam_m", "adam_v", "counters", "metrics")
            else:  # its schedule is done: not touched at all
                inputs += ln.state_names()
        if ctl:
            fn = lambda: lib_.hwy_ppo_sched_ctl_step(ctypes.byref(plan), mem.ptr("table"),  # noqa: E731
                                                     mem.ptr("ctl"), s, stream_ptr())
        else:
            fn = lambda: lib_.hwy_ppo_sched_step(ctypes.byref(plan), mem.ptr("table"), s,  # noqa: E731
                                                 stream_ptr())
        call(mem, f"sched slot {s}", fn, inputs)
        for g, ln in enumerate(ls):
            what = f"sched{'_ctl' if ctl else ''} learner {g} after slot {s}"
            ln.check_slack(poison, what)
            if ctl and g == 0 and s >= trip:
                # the tripping step is dropped: weights, moments and image stay at `trip` applied
                # steps; its metrics row is written and valid, counters = [trip, trip + 1]
                got, want = ln.state(trip + 1), base[0][trip]
                same(got, want, what, keys=("params", "adam_m", "adam_v", "image"))
                assert got["counters"].tolist() == [trip, trip + 1], what
                assert torch.equal(got["metrics"], base[0][trip + 1]["metrics"]), what
            else:
                k = min(s + 1, steps[g])
                same(ln.state(k), base[g][k], what)
    if ctl:
        off = int(lib_.hwy_ppo_sched_ctl_stopped_offset(G)) // 4
        assert mem.words("ctl")[off:off + G].tolist() == [trip, -1, -1]
    call(mem, "sched advance",
         lambda: lib_.hwy_ppo_sched_advance(ctypes.byref(plan), mem.ptr("table"), plan.max_steps,
                                            stream_ptr()), everything)


# ------------------------------------------------------------------ grouped acting
@pytest.mark.parametrize("kind,dims", [("group", GROUP_DIMS), ("mixed", MIXED_DIMS)],
                         ids=["group", "mixed"])
@pytest.mark.parametrize("poison", list(POISONS))
def test_grouped_acting_in_one_arena(poison, kind, dims):
    """hwy_ppo_group_act / hwy_ppo_mixed_act with and without tile images, noise given and NULL:
    each learner's outputs are its solo hwy_ppo_act's on plain allocations."""
    poison = POISONS[poison]
    G, lib_ = len(dims), L()
    base = [run_act(Plain(DEV), B, S, H, None) for B, S, H in dims]
    mem = Arena(DEV)
    acs = [Actor(mem, B, S, H, f"a{g}_") for g, (B, S, H) in enumerate(dims)]
    nb = int(lib_.hwy_ppo_group_act_table_bytes(G) if kind == "group"
             else lib_.hwy_ppo_mixed_act_table_bytes(G))
    assert nb > 0 and nb % 4 == 0
    mem.add("table", nb // 4, 1)
    mem.build()
    for ac in acs:
        ac.load(poison)
        sa = ac.sync_args()
        call(mem, f"{ac.tag} sync_params",
             lambda: lib_.hwy_ppo_sync_params(ctypes.byref(sa), stream_ptr()),
             [n for n in mem.names() if n != ac.tag + "workspace"])
    outs = sum((ac.nm(*Actor.OUT) for ac in acs), [])
    for tiles, noise in ACT_VARIANTS:
        arr = (PpoActArgs * G)()
        for g, ac in enumerate(acs):
            a = ac.args(tiles, noise)
            ctypes.memmove(ctypes.byref(arr[g]), ctypes.byref(a), ctypes.sizeof(PpoActArgs))
            for k in Actor.OUT:
                ac.w(k).fill_(0x7FC54321)
        what = f"{kind} act tiles={tiles} noise={noise}"
        not_table = [n for n in mem.names() if n != "table"]
        if kind == "group":
            d = PpoDims(dims[0][0], max(S for _, S, _ in dims), dims[0][2], 2)
            call(mem, what + " prepare",
                 lambda: lib_.hwy_ppo_group_act_prepare(arr, G, mem.ptr("table"), stream_ptr()),
                 not_table)
            fn = lambda: lib_.hwy_ppo_group_act(ctypes.byref(d), G, tiles, mem.ptr("table"),  # noqa: E731
                                                stream_ptr())
        else:
            plan = PpoMixedActPlan()
            call(mem, what + " prepare",
                 lambda: lib_.hwy_ppo_mixed_act_prepare(arr, G, mem.ptr("table"), ctypes.byref(plan),
                                                        stream_ptr()), not_table)
            fn = lambda: lib_.hwy_ppo_mixed_act(ctypes.byref(plan), mem.ptr("table"), stream_ptr())  # noqa: E731
        call(mem, what, fn, [n for n in mem.names() if n not in outs])
        for g, ac in enumerate(acs):
            same(ac.outputs(), base[g]["act", tiles, noise], f"{what} learner {g}", keys=Actor.OUT)
