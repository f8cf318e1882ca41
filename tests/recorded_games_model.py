"""TEST INFRASTRUCTURE: a plain-Python model of a recorded game (include/synthesis_amd.h "Recorded games"), written from the
definition: tests/selfplay_py.run_game (alpha_zero.rs:229-338: run_game, sample_action, fill_state_info, store_rewards) generalised to
a start position, two players and a record mask. The tree of a ply is the oracle's search of the mover (one root, the mover's blob,
arithmetic, explores, configuration and action selection); the draws are the `Stream`, `gen_range_u8` and `weighted_index` restatements
of tests/frozen_py.py and tests/selfplay_py.py. Outcome kinds are the engine's numbers: 0 = Lose, 1 = Draw, 2 = Win."""
from dataclasses import dataclass

import numpy as np

from tests.frozen_py import F, Game, Stream
from tests.selfplay_py import weighted_index


@dataclass
class Side:
    """one player of a recorded game as the oracle searches for it"""
    blob: np.ndarray
    mcts: object            # tests.oracle_lib.MctsConfig
    explores: int
    action: int = 1         # ActionSelection: 0 = Q, 1 = NumVisits
    nn_mode: int = 1        # oracle.ACC_FMA (the engine's f32) or oracle.ACC_F16X2
    net: str = "mlp"


def record_rules(random_actions_until=0, sample_actions_until=0, stop_games_when_solved=0, value_target=1, vt_p=0.0, vt_from=0.0,
                 vt_to=0.0, record_mask=1):
    return dict(random_actions_until=random_actions_until, sample_actions_until=sample_actions_until,
                stop_games_when_solved=stop_games_when_solved, value_target=value_target, vt_p=vt_p, vt_from=vt_from, vt_to=vt_to,
                record_mask=record_mask)


def rules_of_rollout(cfg, record_mask=1):
    """the rules of a tests.oracle_lib.RolloutConfig (what RecordConfig.from_rollout copies)"""
    return record_rules(cfg.random_actions_until, cfg.sample_actions_until, cfg.stop_games_when_solved, cfg.value_target, cfg.vt_p,
                        cfg.vt_from, cfg.vt_to, record_mask)


def store_reward(value_target, q, z, t, vt_p, vt_from, vt_to):
    """store_rewards (alpha_zero.rs:309-338) for one row, f32 operation by operation"""
    if value_target == 1:
        return np.asarray(q, F)
    if value_target == 0:
        return np.asarray(z, F)
    if value_target == 2:
        p = F(vt_p)
        return np.array([F(F(q[i] * p) + F(z[i] * F(F(1.0) - p))) for i in range(3)], F)
    p = F(F(F(F(1.0) - t) * F(vt_from)) + F(t * F(vt_to)))
    return np.array([F(F(q[i] * F(F(1.0) - p)) + F(z[i] * p)) for i in range(3)], F)


def run_game(oracle, sides, first, second, start_my, start_op, seed, rules):
    """Game g of the definition. Returns dict(plies, rows, row_plies, states, pis, vs, actions, root_nodes, final_kind, moves, reward,
    final_bb, rng_words): the rows' arrays have `rows` entries, moves has `plies`."""
    rng = Stream(oracle, int(seed), 0, budget=4096)
    game, solution, num_turns = Game(int(start_my), int(start_op)), None, 0
    rows, moves = [], []
    while solution is None:
        p = first if num_turns % 2 == 0 else second
        s = sides[p]
        res = oracle.c4_mcts_search(s.mcts, s.blob, [game.my], [game.op], s.explores, action_selection=s.action, nn_mode=s.nn_mode,
                                    net=s.net)
        pi = res["target_pi"][0]
        sol_of = lambda a: int(res["child_sol"][0, a, 1]) if res["child_sol"][0, a, 0] else None  # noqa: E731
        best = int(res["best_action"][0])
        # sample_action (alpha_zero.rs:270-293); turns count from the start position
        if num_turns < rules["random_actions_until"]:
            acts = game.actions()
            action = acts[rng.gen_range_u8(len(acts))]
        elif num_turns < rules["sample_actions_until"] and (sol_of(best) is None or not rules["stop_games_when_solved"]):
            action = weighted_index(rng, pi)
        else:
            action = best
        if (rules["record_mask"] >> p) & 1:
            rows.append(dict(ply=num_turns, state=(game.my, game.op), pi=pi.copy(), q=res["target_q"][0].copy(), action=action,
                             nodes=int(res["num_nodes"][0])))
        moves.append(action)
        solution = sol_of(action)
        game, is_over = game.step(action)
        if is_over:
            solution = 0 if game.reward_for_mover_to_be() < 0 else 1   # the mover made four: Lose for the side to move; else Draw
        elif not rules["stop_games_when_solved"]:
            solution = None
        num_turns += 1
    n = num_turns
    # fill_state_info: the last position's mover (ply n - 1) sees solution.reversed(); one reversal per step back
    last_kind = 2 - solution
    vs = []
    for r in rows:
        kind = last_kind if (n - 1 - r["ply"]) % 2 == 0 else 2 - last_kind
        z = np.zeros(3, F)
        z[kind] = F(1.0)
        t = F(F(r["ply"] + 1) / F(n))
        vs.append(store_reward(rules["value_target"], r["q"], z, t, rules["vt_p"], rules["vt_from"], rules["vt_to"]))
    # the tournament's outputs: the reward of the first mover, the final position as (first mover's stones, second mover's)
    last_mover_first = (n - 1) % 2 == 0
    # (a draw is +0.0 for either mover, as the tournament writes it)
    mover_reward = 0.0 if solution == 1 else (1.0 if solution == 0 else -1.0)
    final_bb = (game.op, game.my) if last_mover_first else (game.my, game.op)
    return dict(plies=n, rows=len(rows), row_plies=[r["ply"] for r in rows], states=[r["state"] for r in rows],
                pis=np.array([r["pi"] for r in rows], F).reshape(-1, 9), vs=np.array(vs, F).reshape(-1, 3),
                actions=[r["action"] for r in rows], root_nodes=[r["nodes"] for r in rows], final_kind=solution, moves=moves,
                reward=F(mover_reward) if last_mover_first else F(F(0.0) - F(mover_reward)), final_bb=final_bb, rng_words=rng.pos)


def run_games(oracle, sides, first, second, start_my, start_op, seeds, rules):
    """the padded arrays Engine.games_run_recorded returns, from run_game per game"""
    n = len(first)
    out = dict(rewards=np.zeros(n, F), plies=np.zeros(n, np.int32), moves=np.full((n, 63), 255, np.uint8), final_bb=np.zeros((n, 2), np.uint64),
               rng_words=np.zeros(n, np.uint64), rows=np.zeros(n, np.int32), states=np.zeros((n, 63, 2), np.uint64),
               pis=np.zeros((n, 63, 9), F), vs=np.zeros((n, 63, 3), F), actions=np.zeros((n, 63), np.uint8),
               root_nodes=np.zeros((n, 63), np.uint32), final_kind=np.zeros(n, np.uint8))
    for g in range(n):
        r = run_game(oracle, sides, int(first[g]), int(second[g]), start_my[g], start_op[g], seeds[g] if seeds is not None else 0, rules)
        k, m = r["rows"], r["plies"]
        out["rewards"][g], out["plies"][g], out["rows"][g], out["final_kind"][g] = r["reward"], m, k, r["final_kind"]
        out["moves"][g, :m] = r["moves"]
        out["final_bb"][g] = r["final_bb"]
        out["rng_words"][g] = r["rng_words"]
        out["states"][g, :k] = np.array(r["states"], np.uint64).reshape(k, 2)
        out["pis"][g, :k], out["vs"][g, :k] = r["pis"], r["vs"]
        out["actions"][g, :k], out["root_nodes"][g, :k] = r["actions"], r["root_nodes"]
    return out


RECORD_KEYS = ("rewards", "plies", "moves", "final_bb", "rng_words", "rows", "states", "pis", "vs", "actions", "root_nodes", "final_kind")


def assert_records_equal(got, want, ctx, keys=RECORD_KEYS):
    """bit for bit, float arrays by their patterns; names the first game that differs"""
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, f"{ctx}: {k} is {a.dtype}{a.shape}, expected {b.dtype}{b.shape}"
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        if not np.array_equal(a, b):
            bad = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=1))
            raise AssertionError(f"{ctx}: {k} differs in {bad.size} games, first game {bad[0]}: {got[k][bad[0]]} vs {want[k][bad[0]]}")
