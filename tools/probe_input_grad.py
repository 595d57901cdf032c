"""Times the input gradients of a policy three ways in one run (development aid):
probe_input_grad.py [out.json]

  input_grad   hwy_ppo_input_grad, the three one-hot cotangents (PPOAgent.input_gradients)
  act          hwy_ppo_act on the same states without a tile image (the forward the kernel runs)
  act_agent    hwy_ppo_act as the agent acts (from its tile image at H = 256)
  autograd     torch autograd on the ActorCritic module: one forward, three backward passes

at B = 4,096 rows, (S, H) = (60, 256) and (600, 384).  Each is captured as a HIP graph of REPS
back-to-back calls, warmed, and replayed ROUNDS times between two events; the figure is the median
replay over REPS, in microseconds per call.  HWY_LIB overrides the library."""
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "highway-rope-ppo_amd"))
import torch
import hwy.native as native

if os.environ.get("HWY_LIB"):
    native.LIB_PATH = os.environ["HWY_LIB"]
from hwy.native import stream_ptr
from hwy.ppo_native import PpoActArgs, PpoDims, _bind, fused_act, fused_input_grad, flat_params, lib
from ppo.agent import PPOAgent
from utils.graphs import capture

dev = torch.device("cuda", 0)
B, REPS, ROUNDS = 4096, 20, 15


def timed(fn):
    """Median microseconds per call of fn over ROUNDS replays of a graph of REPS calls."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with capture(g, stream=side):
            for _ in range(REPS):
                fn()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / REPS * 1e3)
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}


def act_rows(flat, x, H, out):
    a = PpoActArgs()
    a.dims = PpoDims(x.shape[0], x.shape[1], H, 2)
    a.states, a.params = x.data_ptr(), flat.data_ptr()
    a.action, a.pre_tanh, a.logp, a.value = (t.data_ptr() for t in out)
    assert _bind(lib()).hwy_ppo_act(ctypes.byref(a), stream_ptr()) == 0


results = []
for S, H in ((60, 256), (600, 384)):
    torch.manual_seed(0)
    hip = PPOAgent(S, 2, lr=3e-4, hidden_dim=H, device=dev, use_graphs=False, backend="hip")
    tor = PPOAgent(S, 2, lr=3e-4, hidden_dim=H, device=dev, use_graphs=False, backend="torch")
    tor.actor_critic.load_state_dict(hip.actor_critic.state_dict())
    x = torch.randn(B, S, device=dev)
    flat = flat_params(hip)[0]
    cot = torch.eye(3, device=dev).unsqueeze(1).expand(3, B, 3).contiguous()
    out = (torch.empty(B, 2, device=dev), torch.empty(B, 2, device=dev),
           torch.empty(B, device=dev), torch.empty(B, device=dev))
    # agreement with autograd, apart from the rows in which a ReLU decision of the kernel differs
    # from torch fp32's own (a pre-activation within rounding of zero: the gradient jumps there)
    ref = tor.input_gradients(x)
    got, bits = fused_input_grad(hip, x, cot, want_relu_bits=True)
    sh = torch.arange(32, device=dev, dtype=torch.int32)
    mine = ((bits.unsqueeze(-1) >> sh) & 1).bool().reshape(B, 4, H)
    with torch.no_grad():
        m = tor.actor_critic
        z1 = m.shared[0](x)
        z2 = m.shared[2](torch.relu(z1))
        h2 = torch.relu(z2)
        theirs = torch.stack([z1 > 0, z2 > 0, m.actor_mean[0](h2) > 0, m.critic[0](h2) > 0], 1)
    flipped = (mine != theirs).any(dim=(1, 2))
    diff = torch.stack([(got[k] - ref[n]).abs().amax(1) / ref[n].abs().max()
                        for k, n in enumerate(ref)]).amax(0)
    row = {"B": B, "S": S, "H": H, "K": 3, "reps": REPS, "rounds": ROUNDS,
           "rows_with_a_differing_relu_decision": int(flipped.sum()),
           "max_rel_diff_to_autograd_other_rows": diff[~flipped].max().item(),
           "max_rel_diff_to_autograd_those_rows": (diff[flipped].max().item() if flipped.any()
                                                   else None),
           "input_grad": timed(lambda: fused_input_grad(hip, x, cot)),
           "act": timed(lambda: act_rows(flat, x, H, out)),
           "act_agent": timed(lambda: fused_act(hip, x, True, out=out)),
           "autograd": timed(lambda: tor.input_gradients(x))}
    row["input_grad_over_act"] = row["input_grad"]["median_us"] / row["act"]["median_us"]
    row["autograd_over_input_grad"] = row["autograd"]["median_us"] / row["input_grad"]["median_us"]
    print(json.dumps(row), flush=True)
    results.append(row)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(results, f, indent=1)
