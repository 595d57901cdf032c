"""Weight coherence: every way of writing a PPOAgent's weights (the WRITERS), the float64
reference of what the kernels must compute from them afterwards, and the visibility condition
that makes a stale consumer fail (test_weight_coherence.py on the CPU, test_weight_coherence_gpu.py
on the kernels).

A writer takes ``(agent, sd)`` -- ``sd`` the CPU state dict W' of an agent of the same dims built
from another seed -- gets new weights into the agent by one idiom, and returns the agent that now
holds them (the deep copy for ``deepcopy``, else the agent itself).  For the three update writers
the new weights are whatever the update produced.

Everything random is drawn from CPU generators, so a machine with a GPU and one without see the
same bits."""

import contextlib
import copy
import os
import tempfile

import torch

from ppo_ref_util import act64

# (S, H): the 4-wave kernel on the params rows, the 8-wave one, the compact ppo_act_c that always
# streams a tile image, the chunked first layer
SHAPES = ((20, 64), (20, 128), (20, 256), (260, 64))
ROWS = 17
SEED_OLD, SEED_NEW = 11, 23
# log_std is zero in every fresh agent: each seed gets its own, so that a stale one shows
LOG_STD = {SEED_OLD: (-0.4, 0.3), SEED_NEW: (0.2, -0.6)}
# two Adam steps move every weight with a gradient by about 2 LR: far outside the acting
# tolerance, small enough that |pre_tanh| stays where log1p(-tanh^2) is well conditioned
LR = 5e-3
N_UPD, NMB_UPD = 64, 2      # one update: 64 samples in 2 minibatches, 1 epoch
RTOL, ATOL = 1e-4, 2e-5     # the acting tolerance (test_fused_act_matches_actor_critic_act)
VISIBLE = 10.0              # allowances a one-stale-tensor output must be away from the new one

PARAM_NAMES = ("shared.0.weight", "shared.0.bias", "shared.2.weight", "shared.2.bias",
               "actor_mean.0.weight", "actor_mean.0.bias", "actor_mean.2.weight",
               "actor_mean.2.bias", "log_std", "critic.0.weight", "critic.0.bias",
               "critic.2.weight", "critic.2.bias")
ACT_OUTPUTS = ("action", "pre_tanh", "log_prob", "value", "action_det", "pre_tanh_det")
GRAD_OUTPUTS = ("acceleration", "steering", "value")


def feeds(name):
    """The acting outputs a parameter tensor feeds (log_std: the sampled ones only) and the input
    gradients it scales (the biases reach those through the ReLU decisions alone, so none is
    required of them)."""
    if name == "log_std":
        return ("action", "pre_tanh", "log_prob"), ()
    weight = name.endswith("weight")
    if name.startswith("shared"):
        return ACT_OUTPUTS, GRAD_OUTPUTS if weight else ()
    if name.startswith("actor_mean"):
        return (tuple(o for o in ACT_OUTPUTS if o != "value"),
                ("acceleration", "steering") if weight else ())
    return ("value",), ("value",) if weight else ()


def make_agent(S, H, seed, device, use_graphs=False, **kw):
    """A PPOAgent whose weights are PPOAgent's own CPU initialisation under `seed` and whose
    log_std is LOG_STD[seed]; one update is N_UPD samples in NMB_UPD minibatches, one epoch."""
    from ppo.agent import PPOAgent

    torch.manual_seed(seed)
    kw.setdefault("backend", "auto")
    ag = PPOAgent(S, 2, lr=LR, epochs=1, hidden_dim=H, device=torch.device(device),
                  use_graphs=use_graphs, num_minibatches=NMB_UPD, seed=seed, **kw)
    with torch.no_grad():
        ag.actor_critic.log_std.copy_(torch.tensor(LOG_STD[seed]))
    return ag


_SD = {}


def new_state(S, H):
    """W': the CPU state dict of the SEED_NEW agent (computed once per shape; never written)."""
    if (S, H) not in _SD:
        sd = make_agent(S, H, SEED_NEW, "cpu", backend="torch").actor_critic.state_dict()
        _SD[S, H] = {k: v.detach().clone() for k, v in sd.items()}
    return _SD[S, H]


def cpu_state(agent):
    return {k: v.detach().cpu().clone() for k, v in agent.actor_critic.state_dict().items()}


def inputs(S, device="cpu", rows=ROWS):
    """The acting rows, their sampling noise clamped to [-2, 2] (act_case's rule) and the
    truncated / terminated bytes of value_masked (every combination occurs)."""
    g = torch.Generator().manual_seed(1000 + S)
    s = torch.randn(rows, S, generator=g)
    noise = torch.randn(rows, 2, generator=g).clamp(-2.0, 2.0)
    trunc = (torch.arange(rows) % 2 == 0).to(torch.uint8)
    term = (torch.arange(rows) % 3 == 0).to(torch.uint8)
    return tuple(t.to(device).contiguous() for t in (s, noise, trunc, term))


def update_buffer(agent, S, seed=5):
    """A 16 x 4 rollout of drawn states, acted on by the module as it stands (torch forward), with
    drawn rewards: the input of one update.  Returns (buffer, last values, permutation)."""
    from ppo.agent import RolloutBuffer

    T, E = N_UPD // 4, 4
    dev = agent.device
    g = torch.Generator().manual_seed(seed)
    buf = RolloutBuffer(T, E, S, 2, dev)
    buf.states.copy_(torch.randn(T + 1, E, S, generator=g))
    noise = torch.randn(T * E, 2, generator=g).clamp(-2.0, 2.0).to(dev)
    with torch.no_grad():
        a, z, lp, v = agent.actor_critic.act(buf.states[:T].reshape(T * E, S), noise=noise)
    buf.actions.copy_(a.view(T, E, 2))
    buf.pre_tanh.copy_(z.view(T, E, 2))
    buf.log_probs.copy_(lp.view(T, E) + 0.05 * torch.randn(T, E, generator=g).to(dev))
    buf.values.copy_(v.view(T, E))
    buf.rewards.copy_(torch.randn(T, E, generator=g))
    last = torch.randn(E, generator=g).to(dev)
    perm = torch.randperm(T * E, generator=g).to(dev)
    return buf, last, perm


@contextlib.contextmanager
def _torch_path(agent, graphs):
    """update_rollout through the torch learner (eager or graph-replayed) for this one update."""
    keep = agent.backend, agent.use_graphs
    agent.backend, agent.use_graphs = "torch", graphs
    try:
        yield
    finally:
        agent.backend, agent.use_graphs = keep


def fused_update(agent):
    S = agent.actor_critic.shared[0].weight.shape[1]
    buf, last, perm = update_buffer(agent, S)
    agent.update_rollout(buf, last, perm=perm, return_metrics=False)
    assert agent._fused is not None, "the update was not the fused one"
    return agent


# ------------------------------------------------------------------ writers
def _to(agent, sd):
    return {k: v.to(agent.device).clone() for k, v in sd.items()}


def w_load_state_dict(agent, sd):
    agent.actor_critic.load_state_dict(sd)
    return agent


def w_param_copy(agent, sd):
    with torch.no_grad():
        for n, p in agent.actor_critic.named_parameters():
            p.copy_(sd[n])
    return agent


def w_flat_copy(agent, sd):
    from hwy.ppo_native import _PARAM_ORDER, flat_params

    flat, _, offs, _ = flat_params(agent)
    image = flat.detach().clone()
    for n, off in zip(_PARAM_ORDER, offs):
        image[off:off + sd[n].numel()] = sd[n].reshape(-1).to(image.device)
    with torch.no_grad():
        flat.copy_(image)
    return agent


def w_save_load(agent, sd):
    other = make_agent(*_dims(agent), SEED_NEW, agent.device, backend=agent.backend)
    other.actor_critic.load_state_dict(sd)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "w.pt")
        other.save(path)
        agent.load(path)
    return agent


def _torch_update(agent, graphs):
    """update_rollout's torch branch (PPOAgent._run_epochs, every epoch's minibatch steps of the
    torch learner) on drawn advantages and returns: the GAE in front of it is a kernel, and this
    writer also runs in the CPU file."""
    buf, _, perm = update_buffer(agent, _dims(agent)[0])
    n, dev = buf.n, agent.device
    g = torch.Generator().manual_seed(9)
    adv = torch.randn(n, generator=g).to(dev)
    ret = buf.values.reshape(n) + torch.randn(n, generator=g).to(dev)
    half = n // NMB_UPD
    with _torch_path(agent, graphs):
        agent._run_epochs(buf.states[:buf.T].reshape(n, -1), buf.pre_tanh.reshape(n, -1),
                          buf.log_probs.reshape(n), adv, ret,
                          [perm[i * half:(i + 1) * half] for i in range(NMB_UPD)])
    agent.updates += 1
    return agent


def w_torch_eager_update(agent, sd):
    return _torch_update(agent, False)


def w_torch_graph_update(agent, sd):
    return _torch_update(agent, True)


def w_fused_update(agent, sd):
    return fused_update(agent)


def w_data_assign(agent, sd):
    sd = _to(agent, sd)
    for n, p in agent.actor_critic.named_parameters():
        p.data = sd[n]
    return agent


def w_vector_to_parameters(agent, sd):
    ac = agent.actor_critic
    vec = torch.cat([sd[n].reshape(-1) for n, _ in ac.named_parameters()]).to(agent.device)
    torch.nn.utils.vector_to_parameters(vec, ac.parameters())
    return agent


def w_load_assign(agent, sd):
    agent.actor_critic.load_state_dict(_to(agent, sd), assign=True)
    return agent


def w_new_module(agent, sd):
    from ppo.agent import ActorCritic

    S, H = _dims(agent)
    other = ActorCritic(S, 2, H, device=agent.device)
    other.load_state_dict(sd)
    agent.actor_critic = other
    return agent


def w_device_round_trip(agent, sd):
    agent.actor_critic.cpu()
    agent.actor_critic.to(agent.device)
    return w_load_state_dict(agent, sd)


def w_deepcopy(agent, sd):
    return w_load_state_dict(copy.deepcopy(agent), sd)


def w_data_copy(agent, sd):
    for n, p in agent.actor_critic.named_parameters():
        p.data.copy_(sd[n])
    agent.params_written()
    return agent


def w_foreach_data_copy(agent, sd):
    sd = _to(agent, sd)
    named = list(agent.actor_critic.named_parameters())
    torch._foreach_copy_([p.data for _, p in named], [sd[n] for n, _ in named])
    agent.params_written()
    return agent


def _dims(agent):
    w = agent.actor_critic.shared[0].weight
    return w.shape[1], w.shape[0]


# name -> (writer, kind): "seen" needs no further call, "update" likewise with the update's own
# weights, "rebind" gives the parameters other storage, "silent" bumps no counter and calls
# params_written() itself
WRITERS = {
    "a-load_state_dict": (w_load_state_dict, "seen"),
    "b-param_copy": (w_param_copy, "seen"),
    "c-flat_copy": (w_flat_copy, "seen"),
    "d-save_load": (w_save_load, "seen"),
    "e-torch_eager_update": (w_torch_eager_update, "update"),
    "f-torch_graph_update": (w_torch_graph_update, "update"),
    "g-fused_update": (w_fused_update, "update"),
    "h-data_assign": (w_data_assign, "rebind"),
    "i-vector_to_parameters": (w_vector_to_parameters, "rebind"),
    "j-load_assign": (w_load_assign, "rebind"),
    "k-new_module": (w_new_module, "rebind"),
    "l-device_round_trip": (w_device_round_trip, "rebind"),
    "m-deepcopy": (w_deepcopy, "rebind"),
    "n-data_copy": (w_data_copy, "silent"),
    "o-foreach_data_copy": (w_foreach_data_copy, "silent"),
}


# ------------------------------------------------------------------ the float64 reference
def module64(S, H, sd):
    from ppo.agent import ActorCritic

    m = ActorCritic(S, 2, H)
    m.load_state_dict({k: v.detach().cpu() for k, v in sd.items()})
    return m.double()


def outputs64(S, H, sd, s, noise):
    """The float64 acting outputs and input gradients of the weights `sd` on CPU rows."""
    m = module64(S, H, sd)
    with torch.no_grad():
        a, z, lp, v = m.act(s.double(), noise=noise.double())
        ad, zd, _, _ = m.act(s.double(), deterministic=True)
    x = s.double().clone().requires_grad_(True)
    mean, _, value = m(x)
    grads = [torch.autograd.grad(o, x, retain_graph=True)[0]
             for o in (mean[:, 0].sum(), mean[:, 1].sum(), value.sum())]
    out = dict(zip(ACT_OUTPUTS, (a, z, lp, v, ad, zd)))
    out.update({"d_" + n: g for n, g in zip(GRAD_OUTPUTS, grads)})
    return out


def assert_visible(S, H, old_sd, new_sd, s, noise, names=PARAM_NAMES):
    """The visibility condition, on the reference alone: with any one parameter tensor left at its
    old value, every output it feeds is at least VISIBLE allowances from the all-new output on at
    least one row -- acting outputs at ATOL + RTOL |ref|, input gradients at the gradient test's
    2e-5 max|ref| + 1e-3 |ref| -- so a kernel that read one stale tensor, whose result lies within
    one allowance of the stale reference, misses the new reference by VISIBLE - 1 of them.
    Returns the smallest margin found, in allowances."""
    s, noise = s.cpu(), noise.cpu()
    new = outputs64(S, H, new_sd, s, noise)
    worst = float("inf")
    for name in names:
        stale_sd = dict(new_sd)
        stale_sd[name] = old_sd[name]
        stale = outputs64(S, H, stale_sd, s, noise)
        acts, grads = feeds(name)
        for o in acts:
            far = ((stale[o] - new[o]).abs() / (ATOL + RTOL * new[o].abs())).max().item()
            assert far >= VISIBLE, (S, H, name, o, far)
            worst = min(worst, far)
        for o in grads:
            ref = new["d_" + o]
            allow = 2e-5 * ref.abs().max() + 1e-3 * ref.abs()
            far = ((stale["d_" + o] - ref).abs() / allow).max().item()
            assert far >= VISIBLE, (S, H, name, "d_" + o, far)
            worst = min(worst, far)
    return worst


def check_acting(agent, s, noise, msg=""):
    """select_action (sampled with `noise`, deterministic) and value against act64 of the module
    as it stands, at the acting tolerance.  Returns the kernel's outputs."""
    ref, ref_d = act64(agent, s, noise)
    with torch.no_grad():
        got = agent.select_action(s, noise=noise)
        got_d = agent.select_action(s, deterministic=True)
        val = agent.value(s)
    names = ("action", "pre_tanh", "log_prob", "value")
    for tag, gs, rs in (("sampled", got, ref), ("deterministic", got_d, ref_d)):
        for n, g, r in zip(names, gs, rs):
            torch.testing.assert_close(g.double(), r.to(g.device), rtol=RTOL, atol=ATOL,
                                       msg=lambda m, n=n, tag=tag: f"{msg} {tag} {n}: {m}")
    torch.testing.assert_close(val.double(), ref_d[3].to(val.device), rtol=RTOL, atol=ATOL,
                               msg=lambda m: f"{msg} value(): {m}")
    return tuple(t.clone() for t in got + got_d + (val,))
