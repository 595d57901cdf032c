"""episode_schedule="reference" (ppo/rollout.py, ppo/group.py, training/routine.py): with one env
and T = steps_per_update the vectorised path runs the reference's own collection loop
(reference training/routine.py:121-243) -- episodes cut at the update boundary and restarted
with seed exp_seed + episode_num, evaluations ahead of the update -- grouped runs equal solo
ones, and the default schedule is untouched."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HORIZON = 10


def _make(seed, autoreset=True):
    from config.base_config import HIGHWAY_CONFIG
    from experiments.config import Condition
    from experiments.wrappers import make_env

    env = make_env(Condition.SORTED, HIGHWAY_CONFIG,
                   env_overrides={"max_episode_steps": HORIZON, "num_envs": 1, "vector_env": True,
                                  "device": DEV, "autoreset": autoreset})
    return env.unwrapped


@pytest.mark.parametrize("spu", [24, 20])
def test_one_env_stream_replays_as_the_reference_collection_loop(spu):
    """spu 24: episodes of 10, 10 and a cut one of 4 steps per collection; spu 20: an
    untruncated stream ends exactly on the boundary, so there is nothing to cut."""
    from hwy import _abi
    from ppo.agent import PPOAgent, RolloutBuffer
    from ppo.rollout import LockstepRollout
    from training.routine import _episode_stream
    from utils.reproducibility import set_random_seeds

    exp_seed, iters = 42, 2
    set_random_seeds(exp_seed)
    env = _make(exp_seed)
    sd = env.obs_rows * env.obs_features
    agent = PPOAgent(sd, 2, device=DEV, lr=3e-4, epochs=2, batch_size=8, hidden_dim=64)
    buf = RolloutBuffer(spu, 1, sd, 2, DEV)
    env.set_seed_schedule(exp_seed)
    obs, _ = env.reset()
    buf.states[0].copy_(obs.reshape(1, sd))
    roll = LockstepRollout(agent, env, buf, episode_schedule="reference")
    tape, streams = [], []
    for _ in range(iters):
        roll.run()
        tape.append({k: getattr(buf, k).clone().cpu() for k in
                     ("states", "actions", "rewards", "dones", "terminated", "truncated")})
        tape[-1].update(cut=roll.cut.clone().cpu(), cut_length=roll.cut_length.clone().cpu(),
                        next0=roll.next0.clone().cpu())
        streams.append(_episode_stream(buf.dones, buf.ep_return, roll.cut, roll.cut_return))
        agent.update_rollout(buf, agent.value(buf.states[spu]))
        roll.start_next()
    torch.cuda.synchronize()
    words = env.export_state().cpu().numpy().view(np.uint32)[_abi.F_ENV, 0]

    # the reference loop (routine.py:121-156) restated on a one-env handle without autoreset,
    # fed the taped actions
    ref = _make(exp_seed, autoreset=False)
    episode_num, crashes = 0, 0
    try:
        for it in range(iters):
            rec = tape[it]
            steps, episodes, done = 0, [], True
            while steps < spu:
                episode_num += 1
                o, _ = ref.reset(seeds=torch.tensor([exp_seed + episode_num]))
                o = o.clone()
                ep_reward, done = np.float32(0.0), False
                while not done and steps < spu:
                    assert torch.equal(rec["states"][steps, 0], o.reshape(-1).cpu()), (it, steps)
                    o, r, te, tr, _ = ref.step(rec["actions"][steps].to(DEV))
                    o = o.clone()
                    done = bool(te.item()) or bool(tr.item())
                    crashes += bool(te.item())
                    assert float(r.item()) == float(rec["rewards"][steps, 0]), (it, steps)
                    last = steps == spu - 1
                    # the cut step's dones is 0: GAE bootstraps it with V(states[T])
                    assert int(rec["dones"][steps, 0]) == int(done), (it, steps)
                    assert int(rec["terminated"][steps, 0] | rec["truncated"][steps, 0]) == int(done)
                    ep_reward = np.float32(ep_reward + np.float32(r.item()))
                    steps += 1
                    if last and not done:
                        assert int(rec["cut"][0]) == 1
                        assert int(rec["cut_length"][0]) > 0
                        # the bootstrap state is the unfinished episode's last observation
                        assert torch.equal(rec["states"][spu, 0], o.reshape(-1).cpu())
                episodes.append(float(ep_reward))
            if done:  # the stream ended on the boundary: nothing was cut
                assert int(rec["cut"][0]) == 0 and int(rec["cut_length"][0]) == 0
                assert torch.equal(rec["next0"], rec["states"][spu])
            assert streams[it].tolist() == episodes, it
        # the numbering: the running episode is the reference's next one, with its seed
        assert int(words[_abi.E_EPISODE]) + 1 == episode_num + 1
        seed = int(words[_abi.E_SEED_LO]) | (int(words[_abi.E_SEED_HI]) << 32)
        assert seed == exp_seed + episode_num + 1
        if spu == 20 and crashes == 0:
            assert [len(s) for s in streams] == [2, 2] and int(tape[-1]["cut"][0]) == 0
        if spu == 24 and crashes == 0:
            assert [len(s) for s in streams] == [3, 3] and int(tape[-1]["cut_length"][0]) == 4
    finally:
        env.close()
        ref.close()


def _exp(seed, cond_name="SORTED", H=64, d=None, name="rs", **extra):
    from experiments.config import Condition, ConditionHP, Experiment

    hp = ConditionHP(lr=3e-4, clip_eps=0.2, epochs=2, batch_size=8, hidden_dim=H, d_embed=d)
    hp.entropy_coef = 0.005
    hp.steps_per_update = 24
    ex = {"num_envs": 1, "episode_schedule": "reference", "eval_interval": 4, "log_interval": 50}
    ex.update(extra)
    ex = {k: v for k, v in ex.items() if v is not None}
    return Experiment(name=f"{name}_{cond_name}_{H}_{seed}", condition=Condition[cond_name], hp=hp,
                      seed=seed, max_episodes=12, target_reward=1e9, extra=ex,
                      env_config_overrides={"max_episode_steps": HORIZON})


def _same_status(a, b):
    assert a["status"] == b["status"] == "COMPLETED", (a.get("error_message"),
                                                       b.get("error_message"))
    assert a["rewards"] == b["rewards"] and a["avg_rewards"] == b["avg_rewards"]
    ma, mb = a["metrics_history"], b["metrics_history"]
    assert ma["episode_rewards"] == mb["episode_rewards"]
    assert ma["eval_episode_numbers"] == mb["eval_episode_numbers"]
    assert [u["loss"] for u in ma["policy_updates"]] == [u["loss"] for u in mb["policy_updates"]]
    assert [u["episode"] for u in ma["policy_updates"]] == [u["episode"] for u in mb["policy_updates"]]


def test_evaluations_run_before_the_update(tmp_path, monkeypatch):
    """An evaluation that falls in the first collection sees the initial weights: it repeats the
    initial evaluation exactly (same weights, same seeds) -- only if it precedes the update."""
    from config.base_config import HIGHWAY_CONFIG
    from experiments.runner import ExperimentRunner

    monkeypatch.chdir(tmp_path)
    res = ExperimentRunner(HIGHWAY_CONFIG).launch(_exp(42, eval_interval=2))
    assert res["status"] == "COMPLETED", res.get("error_message")
    mh = res["metrics_history"]
    assert mh["eval_episode_numbers"][:2] == [0, 2]
    assert mh["eval_rewards"][1] == mh["eval_rewards"][0]
    assert len(set(mh["eval_rewards"])) > 1  # later evaluations see updated weights
    # 24 steps per collection at a horizon of 10: at least three episodes per update
    assert all(u["steps"] == 24 for u in mh["policy_updates"])
    assert mh["policy_updates"][0]["episode"] >= 3 and len(mh["episode_rewards"]) == 12


def test_launch_group_equals_launch_on_the_reference_schedule(tmp_path, monkeypatch):
    from config.base_config import HIGHWAY_CONFIG
    from experiments.runner import ExperimentRunner

    monkeypatch.chdir(tmp_path)
    seeds = [42, 1042, 7]
    grouped = ExperimentRunner(HIGHWAY_CONFIG).launch_group([_exp(s) for s in seeds])
    for s, g in zip(seeds, grouped):
        _same_status(ExperimentRunner(HIGHWAY_CONFIG).launch(_exp(s)), g)


def test_launch_batch_equals_launch_group_on_the_reference_schedule(tmp_path, monkeypatch):
    from config.base_config import HIGHWAY_CONFIG
    from experiments.runner import ExperimentRunner

    monkeypatch.chdir(tmp_path)
    cells = [[_exp(s, "SHUFFLED_RANKPE", 128, 4) for s in (42, 1042)],
             [_exp(s, "SORTED", 256) for s in (7, 2042)]]
    batched = ExperimentRunner(HIGHWAY_CONFIG).launch_batch(cells)
    for cell, got in zip(cells, batched):
        alone = ExperimentRunner(HIGHWAY_CONFIG).launch_group(cell)
        for a, b in zip(alone, got):
            _same_status(a, b)


def test_lockstep_schedule_is_the_path_without_the_keyword(tmp_path, monkeypatch):
    """extra["episode_schedule"] = "lockstep" runs exactly what a run that never names the
    schedule runs: no rollout, group or training loop is handed the keyword."""
    import ppo.group
    import ppo.rollout
    from config.base_config import HIGHWAY_CONFIG
    from experiments.runner import ExperimentRunner

    monkeypatch.chdir(tmp_path)
    seen = []
    for cls in (ppo.rollout.LockstepRollout, ppo.group.ExperimentGroup):
        init = cls.__init__

        def spy(self, *a, _init=init, **kw):
            seen.append(sorted(kw))
            _init(self, *a, **kw)

        monkeypatch.setattr(cls, "__init__", spy)
    out = []
    for schedule in ("lockstep", None):
        kw = dict(num_envs=4, episode_schedule=schedule)
        solo = ExperimentRunner(HIGHWAY_CONFIG).launch(_exp(42, name=f"l{schedule}", **kw))
        grp = ExperimentRunner(HIGHWAY_CONFIG).launch_group(
            [_exp(s, name=f"g{schedule}", **kw) for s in (42, 1042)])
        out.append([solo] + grp)
    assert seen and not any("episode_schedule" in kw for kw in seen)
    for a, b in zip(*out):
        _same_status(a, b)
    _same_status(out[0][0], out[0][1])  # and the grouped run is the solo run, as before


def test_long_rollout_chunk_graphs_equal_eager():
    """A reference rollout longer than REFERENCE_GRAPH_CHUNK steps is issued as one graph per
    chunk (the cut in the last); solo and grouped, it gives what the eager launches give."""
    from config.base_config import HIGHWAY_CONFIG
    from experiments.config import Condition
    from ppo.agent import PPOAgent, RolloutBuffer
    from ppo.group import build_group
    from ppo.rollout import REFERENCE_GRAPH_CHUNK, LockstepRollout, rollout_chunks
    from utils.reproducibility import set_random_seeds

    T, iters, seed = REFERENCE_GRAPH_CHUNK + 64, 4, 42  # 5 minibatches of 64
    assert len(rollout_chunks(T, "reference")) == 2
    keys = ("states", "actions", "rewards", "dones", "log_probs", "values")

    def agent_for(sd):
        return PPOAgent(sd, 2, device=DEV, lr=3e-4, epochs=2, batch_size=64, hidden_dim=64)

    def solo(graphs):
        set_random_seeds(seed)
        env = _make(seed)
        sd = env.obs_rows * env.obs_features
        agent = agent_for(sd)
        buf = RolloutBuffer(T, 1, sd, 2, DEV)
        env.set_seed_schedule(seed)
        obs, _ = env.reset()
        buf.states[0].copy_(obs.reshape(1, sd))
        roll = LockstepRollout(agent, env, buf, use_graph=graphs, episode_schedule="reference")
        hist = []
        for _ in range(iters):
            roll.run()
            hist.append([getattr(buf, k).clone() for k in keys]
                        + [roll.next0.clone(), roll.cut.clone(), roll.cut_return.clone()])
            agent.update_rollout(buf, agent.value(buf.states[T]))
            roll.start_next()
        torch.cuda.synchronize()
        env.close()
        return hist, dict(roll.stats)

    def grouped(graphs):
        grp = build_group(Condition.SORTED, HIGHWAY_CONFIG, [seed, 1042], 1, T, DEV, agent_for,
                          env_overrides={"max_episode_steps": HORIZON}, use_graphs=graphs,
                          episode_schedule="reference")
        hist = []
        for _ in range(iters):
            grp.rollout()
            hist.append([getattr(grp.buf, k).clone() for k in keys]
                        + [grp.next0.clone(), grp.cut.clone(), grp.cut_return.clone()])
            grp.update()
        torch.cuda.synchronize()
        stats = dict(grp.stats)
        grp.close()
        return hist, stats

    for run in (solo, grouped):
        (hg, sg), (he, _) = run(True), run(False)
        assert sg["rollout_capture"] >= 2 and sg["rollout_replay"] >= 2, sg  # both chunks
        for it in range(iters):
            for a, b in zip(hg[it], he[it]):
                assert torch.equal(a, b), (run.__name__, it)


@pytest.mark.parametrize("H", [64, 128])
def test_group_equals_solo_at_one_env_and_a_long_rollout(H):
    """G = 2 experiments of one env each, T = 320 (two chunk graphs, 5 minibatches of 64): every
    rollout row, every update's metrics, the final weights and Adam moments equal the solo
    LockstepRollout + update_rollout run.  With E = 1 an experiment's [T, 1] slice of the grouped
    advantages reshapes to a strided view; the group normalises a contiguous copy, as the solo
    run does, or torch sums it in another order and the runs part at the first update."""
    from config.base_config import HIGHWAY_CONFIG
    from experiments.config import Condition
    from ppo.agent import PPOAgent, RolloutBuffer
    from ppo.group import build_group
    from ppo.rollout import LockstepRollout
    from utils.reproducibility import set_random_seeds

    T, iters, seeds = 320, 3, [42, 1042]
    keys = ("states", "actions", "rewards", "dones", "log_probs", "values")

    def agent_for(sd):
        return PPOAgent(sd, 2, device=DEV, lr=3e-4, epochs=2, batch_size=64, hidden_dim=H)

    grp = build_group(Condition.SORTED, HIGHWAY_CONFIG, seeds, 1, T, DEV, agent_for,
                      env_overrides={"max_episode_steps": HORIZON}, episode_schedule="reference")
    ghist, gmet = [], []
    for _ in range(iters):
        grp.rollout()
        ghist.append([getattr(grp.buf, k).clone() for k in keys]
                     + [grp.next0.clone(), grp.cut_return.clone()])
        gmet.append(grp.update())
    torch.cuda.synchronize()
    for g, seed in enumerate(seeds):
        set_random_seeds(seed)
        env = _make(seed)
        sd = env.obs_rows * env.obs_features
        agent = agent_for(sd)
        buf = RolloutBuffer(T, 1, sd, 2, DEV)
        env.set_seed_schedule(seed)
        obs, _ = env.reset()
        buf.states[0].copy_(obs.reshape(1, sd))
        roll = LockstepRollout(agent, env, buf, episode_schedule="reference")
        for it in range(iters):
            roll.run()
            solo = [getattr(buf, k) for k in keys]
            for k, a, b in zip(keys, solo, ghist[it][:6]):
                assert torch.equal(a, b[:, g:g + 1]), (g, it, k)
            assert torch.equal(roll.next0, ghist[it][6][g:g + 1]), (g, it)
            assert torch.equal(roll.cut_return, ghist[it][7][g:g + 1]), (g, it)
            m = agent.update_rollout(buf, agent.value(buf.states[T]))
            assert m == gmet[it][g], (g, it)
            roll.start_next()
        torch.cuda.synchronize()
        for (k, va), (_, vb) in zip(agent.actor_critic.state_dict().items(),
                                    grp.agents[g].actor_critic.state_dict().items()):
            assert torch.equal(va, vb), (g, k)
        Fs, Fg = agent._fused, grp.agents[g]._fused
        assert torch.equal(Fs.m, Fg.m) and torch.equal(Fs.v, Fg.v), g
        env.close()
    grp.close()
