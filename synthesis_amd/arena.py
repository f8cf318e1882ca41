"""Which of two checkpoints is stronger, with an error bar: many games between two networks on the device (Engine.match_run =
syn_match_run), from many different openings, each opening played once per colour.

Two network players under ActionSelection::NumVisits and Fpu::Const are deterministic, so every game from the empty board is the same
game; the information is in the openings. `random_openings` draws them, `compare` plays every opening twice (A first, B first: ONE
match_run call per colour) and reduces the results to a score with its standard error over openings and the Elo difference that score
implies. `host_match` is the same match on the host path of match.play_match (one mcts_search per ply, numpy steps), from given
starts: what the device match is timed and tested against. A player may name an `.arithmetic` of its own ("f32" / "f16x2"): `compare`
then plays through Engine.match_run_sides, so one checkpoint can meet itself in the other arithmetic; `compare_baseline` plays a
checkpoint against the evaluator's VanillaMCTS<n> (match.vanilla_player) with the same statistics.

More than two players: `tournament` / `round_robin` / `gauntlet` play every pair of a schedule on every opening, once per colour, in ONE
Engine.tournament_run (syn_tournament_run: one device-resident loop, one search launch per player and ply) and return compare's
statistics per pair; `ratings` puts the pairs on one scale (maximum-likelihood Bradley-Terry strengths as Elo, bootstrap intervals
over openings).

Host code only draws openings and does statistics — no search, no network."""
import math

import numpy as np

from . import match

_U = np.uint64
_COL = _U(0x7F)


def mirror(bb):
    """left-right mirror image of bitboards (bit = row + 7 * col: column c <-> column 8 - c)"""
    bb = np.asarray(bb, np.uint64)
    out = np.zeros(bb.shape, np.uint64)
    for c in range(9):
        out |= ((bb >> _U(7 * c)) & _COL) << _U(7 * (8 - c))
    return out


def _heights(occ):
    """stones per column, [n, 9]"""
    cols = (occ[:, None] >> (_U(7) * np.arange(9, dtype=np.uint64))[None, :]) & _COL
    h = np.zeros(cols.shape, np.int64)
    for r in range(7):
        h += ((cols >> _U(r)) & _U(1)).astype(np.int64)
    return h


def random_openings(n, plies, seed, max_rounds=32):
    """n start positions (my, op: uint64 arrays, the stones of the player to move first), each reached from the empty board by `plies`
    uniformly random legal moves; none is won or full, and no two are equal or mirror images of each other.

    The draw, so that a seed names a set of openings: rng = numpy.random.default_rng(seed) (PCG64). Candidates come in rounds of
    2 * n + 64 games played side by side; at every ply ONE rng.random(size) call gives each game a u in [0, 1), and the game plays its
    floor(u * L)-th legal column in ascending order, L = its number of legal columns. A candidate that ended on the way (four in a row,
    or a full board) is dropped. Survivors are taken in candidate order; one whose position or mirror image was taken before is
    skipped. Raises ValueError when n distinct openings have not been found after max_rounds rounds (too few reachable positions at
    that depth: at 2 plies there are 45 up to mirror)."""
    n, plies = int(n), int(plies)
    if n < 0 or plies < 0 or plies > 62:
        raise ValueError("random_openings: need n >= 0 and 0 <= plies <= 62")
    rng = np.random.default_rng(seed)
    size = 2 * n + 64
    seen, out_my, out_op = set(), [], []
    for _ in range(max_rounds):
        if len(out_my) >= n:
            break
        my = np.zeros(size, np.uint64); op = np.zeros(size, np.uint64)
        alive = np.ones(size, bool)
        for _ply in range(plies):
            u = rng.random(size)
            legal = _heights(my | op) < 7
            count = legal.sum(axis=1)
            k = np.minimum((u * count).astype(np.int64), np.maximum(count - 1, 0))
            col = ((np.cumsum(legal, axis=1) - 1 == k[:, None]) & legal).argmax(axis=1)
            my, op, over, _w = match.step(my, op, col)
            alive &= ~over & (count > 0)
        m_my, m_op = mirror(my), mirror(op)
        for i in np.nonzero(alive)[0]:
            a, b = (int(my[i]), int(op[i])), (int(m_my[i]), int(m_op[i]))
            key = min(a, b)
            if key in seen:
                continue
            seen.add(key)
            out_my.append(a[0]); out_op.append(a[1])
            if len(out_my) >= n:
                break
    if len(out_my) < n:
        raise ValueError(f"random_openings: only {len(out_my)} distinct openings of {plies} plies after {max_rounds} rounds of {size} draws, {n} wanted")
    return np.array(out_my[:n], np.uint64), np.array(out_op[:n], np.uint64)


def elo(score):
    """Elo difference implied by a score in [0, 1], clipped as match.score clips (to [1e-3, 1 - 1e-3])"""
    s = min(max(float(score), 1e-3), 1 - 1e-3)
    return float(-400.0 * math.log10(1.0 / s - 1.0))


def pair_statistics(rewards_a_first, rewards_b_first):
    """The statistics of `compare` from the two reward vectors alone. rewards_a_first[o]: the first mover's reward (+1 / 0 / -1) in
    opening o's game with A moving first; rewards_b_first[o]: the first mover's reward in the game with B moving first (so A scores
    its negative). p_o = mean of A's two game scores (win 1, draw 1/2, loss 0), in {0, 1/4, 1/2, 3/4, 1}: the unit of the error bar is
    the opening, because the two games of an opening are not independent. S = mean(p_o), SE = std(p_o, ddof=1) / sqrt(n) (nan for
    fewer than two openings); the Elo difference of S and of S -/+ 1.96 SE."""
    r1 = np.asarray(rewards_a_first, np.float64).ravel()
    r2 = np.asarray(rewards_b_first, np.float64).ravel()
    if r1.size != r2.size:
        raise ValueError("pair_statistics: one reward per opening and colour")
    n = int(r1.size)
    p = ((1.0 + r1) / 2.0 + (1.0 - r2) / 2.0) / 2.0
    s = float(p.mean()) if n else float("nan")
    se = float(p.std(ddof=1) / math.sqrt(n)) if n >= 2 else float("nan")
    lo, hi = s - 1.96 * se, s + 1.96 * se
    fin = lambda x: elo(x) if x == x else float("nan")  # noqa: E731
    return dict(openings=n,
                wins=int((r1 > 0).sum() + (r2 < 0).sum()), draws=int((r1 == 0).sum() + (r2 == 0).sum()),
                losses=int((r1 < 0).sum() + (r2 > 0).sum()),
                pair_scores=p, score=s, se=se, score_lo=lo, score_hi=hi, elo=fin(s), elo_lo=fin(lo), elo_hi=fin(hi))


class _Side:
    """a player's search settings with a blob of its own: what Engine.match_run_sides takes as a network side"""
    frozen = False
    rollout = False

    def __init__(self, player, blob):
        self.explores, self.action, self.mcts_cfg = player.explores, player.action, player.mcts_cfg
        self.arithmetic = getattr(player, "arithmetic", None)
        self.weights = blob


def _match(engine, first, second, blob_first, blob_second, my, op):
    """one colour of `compare`: Engine.match_run, or Engine.match_run_sides when a player names an arithmetic of its own"""
    if getattr(first, "arithmetic", None) is None and getattr(second, "arithmetic", None) is None:
        return engine.match_run(first, second, blob_first, blob_second, my, op)
    return engine.match_run_sides(_Side(first, blob_first), _Side(second, blob_second), my, op)


def compare(engine, blob_a, blob_b, openings, player_a, player_b):
    """Network A (blob_a, searched as player_a says) against network B on every opening, once with A moving first and once with B:
    two device matches, all games of a colour in one. `openings` = (my, op) as random_openings returns them; the players are
    anything with .explores, .action and .mcts_cfg (match.Player) and an optional .arithmetic (None: the engine's, "f32", "f16x2" —
    the same blob for both players and two arithmetics is one checkpoint against itself in the other arithmetic). Returns
    pair_statistics' dict (W/D/L from A's side) plus "plies_a_first" / "plies_b_first"."""
    my, op = openings
    g1 = _match(engine, player_a, player_b, blob_a, blob_b, my, op)
    g2 = _match(engine, player_b, player_a, blob_b, blob_a, my, op)
    out = pair_statistics(g1["rewards"], g2["rewards"])
    out["plies_a_first"], out["plies_b_first"] = g1["plies"], g2["plies"]
    return out


def compare_baseline(engine, blob_a, openings, player_a, baseline, seeds):
    """Network A against the evaluator's baseline (match.vanilla_player) on every opening, both colours, game o of either colour on
    StdRng::seed_from_u64(seeds[o]): the absolute anchor of the reference's evaluator (eval_against_rollout_mcts) with compare's
    statistics. Returns compare's dict."""
    my, op = openings
    a = _Side(player_a, blob_a)
    g1 = engine.match_run_sides(a, baseline, my, op, seeds=seeds)
    g2 = engine.match_run_sides(baseline, a, my, op, seeds=seeds)
    out = pair_statistics(g1["rewards"], g2["rewards"])
    out["plies_a_first"], out["plies_b_first"] = g1["plies"], g2["plies"]
    return out


# ---- more than two players: one device-resident tournament (Engine.tournament_run = syn_tournament_run) and a rating fit
def round_robin_pairs(n_players):
    """every unordered pair (a, b), a < b, in ascending order"""
    return [(a, b) for a in range(int(n_players)) for b in range(a + 1, int(n_players))]


def gauntlet_pairs(n_candidates, n_anchors):
    """every candidate (players 0 .. n_candidates - 1) with every anchor (the players after them), and no other pair"""
    return [(c, int(n_candidates) + a) for c in range(int(n_candidates)) for a in range(int(n_anchors))]


def schedule(pairs, n_openings, n_players=None):
    """The games of a tournament: for every opening (outer loop) and every pair (a, b) of `pairs` two games, a moving first, then b
    moving first — interleaved by opening, not grouped by pairing. Returns dict(first, second, opening, pair [n_games], a_first
    [n_games] bool, pairs). Raises ValueError on a pair named twice (in either order), a self-pairing or an index out of range."""
    pairs = [(int(a), int(b)) for a, b in pairs]
    seen = set()
    for a, b in pairs:
        if a == b or a < 0 or b < 0 or (n_players is not None and max(a, b) >= n_players):
            raise ValueError(f"schedule: pair ({a}, {b}) is a self-pairing or names a player that does not exist")
        if (min(a, b), max(a, b)) in seen:
            raise ValueError(f"schedule: pair ({a}, {b}) is named twice")
        seen.add((min(a, b), max(a, b)))
    n_openings, m = int(n_openings), len(pairs)
    pa = np.array([p[0] for p in pairs], np.int32).reshape(m)
    pb = np.array([p[1] for p in pairs], np.int32).reshape(m)
    one = np.stack([np.stack([pa, pb], 1), np.stack([pb, pa], 1)], 1).reshape(2 * m, 2)   # per opening: (a, b), (b, a) per pair
    first = np.tile(one[:, 0], n_openings).astype(np.int32)
    second = np.tile(one[:, 1], n_openings).astype(np.int32)
    return dict(first=first, second=second, opening=np.repeat(np.arange(n_openings, dtype=np.int64), 2 * m),
                pair=np.tile(np.repeat(np.arange(m, dtype=np.int64), 2), n_openings),
                a_first=np.tile(np.array([True, False] * m, bool), n_openings), pairs=pairs)


def tournament(engine, players, pairs, openings, seeds=None):
    """Every pair of `pairs` on every opening, once per colour, all games in ONE Engine.tournament_run. `players`: what
    Engine.match_run_sides takes as sides (a network player carries its own .weights and an optional .arithmetic; match.vanilla_player is
    a baseline); `seeds` [n_openings]: game o of either colour of every pair plays on StdRng::seed_from_u64(seeds[o]), as in
    compare_baseline (needed when a player is a baseline). Returns dict(n_players, pairs, stats = {pair: pair_statistics' dict from that
    pair's two reward vectors plus "plies_a_first" / "plies_b_first" — compare's numbers for the pair}, games = tournament_run's raw
    arrays, schedule)."""
    my, op = (np.asarray(x, np.uint64).ravel() for x in openings)
    sch = schedule(pairs, my.size, len(players))
    o = sch["opening"]
    game_seeds = None if seeds is None else np.asarray(seeds, np.uint64).ravel()[o]
    games = engine.tournament_run(players, sch["first"], sch["second"], my[o], op[o], seeds=game_seeds)
    stats = {}
    for j, pair in enumerate(sch["pairs"]):
        g1 = np.nonzero((sch["pair"] == j) & sch["a_first"])[0]      # (in opening order)
        g2 = np.nonzero((sch["pair"] == j) & ~sch["a_first"])[0]
        st = pair_statistics(games["rewards"][g1], games["rewards"][g2])
        st["plies_a_first"], st["plies_b_first"] = games["plies"][g1], games["plies"][g2]
        stats[pair] = st
    return dict(n_players=len(players), pairs=sch["pairs"], stats=stats, games=games, schedule=sch)


def round_robin(engine, players, openings, seeds=None):
    """`tournament` over all pairs"""
    return tournament(engine, players, round_robin_pairs(len(players)), openings, seeds=seeds)


def gauntlet(engine, candidates, anchors, openings, seeds=None):
    """`tournament` of every candidate against every anchor only; the players are candidates + anchors, in that order"""
    players = list(candidates) + list(anchors)
    return tournament(engine, players, gauntlet_pairs(len(candidates), len(anchors)), openings, seeds=seeds)


def results_from_pair_scores(n_players, pair_scores):
    """What `ratings` reads of a tournament's return value, from {(a, b): p_o per opening} alone (p_o = a's mean score of the opening's
    two games, as pair_statistics defines it): for recorded or synthetic results."""
    pairs = [(int(a), int(b)) for a, b in pair_scores]
    return dict(n_players=int(n_players), pairs=pairs,
                stats={p: dict(pair_scores=np.asarray(v, np.float64).ravel()) for p, v in zip(pairs, pair_scores.values())})


def _bradley_terry(S, N, tol=1e-13, max_iter=200000):
    """MM iteration gamma_i <- S_i / sum_j n_ij / (gamma_i + gamma_j) for a batch: S [B, K] total scores, N [B, K, K] games per pair
    (symmetric, zero diagonal). Returns gamma [B, K] (geometric mean 1 over each row's positive entries) and the iterations taken."""
    B, K = S.shape
    g = np.ones((B, K))
    it = 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for it in range(1, max_iter + 1):
            den = (N / (g[:, :, None] + g[:, None, :])).sum(axis=2)
            new = np.where(den > 0, S / den, g)
            pos = new > 0
            logs = np.where(pos, np.log(np.where(pos, new, 1.0)), 0.0)
            new = np.where(pos, new / np.exp(logs.sum(axis=1, keepdims=True) / np.maximum(pos.sum(axis=1, keepdims=True), 1)), 0.0)
            change = np.where(pos & (g > 0), np.abs(np.log(np.where(pos, new, 1.0)) - np.log(np.where(g > 0, g, 1.0))), 0.0)
            g = new
            if not np.isfinite(g).all() or change.max() < tol:
                break
    return g, it


def ratings(results, anchor=0, prior_draws=0.0, bootstrap=400, seed=0):
    """Maximum-likelihood Bradley-Terry strengths of a tournament's players, as Elo relative to player `anchor`:
    400 * log10(gamma_i / gamma_anchor), fitted on game scores (a draw counts as half a win) by the MM iteration
    gamma_i <- S_i / sum_j n_ij / (gamma_i + gamma_j). `prior_draws` adds that many virtual drawn games to every played pair.
    With prior_draws == 0 a player whose total score is 0 or maximal, or a pairing graph that is not connected, has no finite maximum:
    ValueError naming the player or the component.
    Intervals: the 2.5 / 97.5 percentiles of `bootstrap` refits over openings resampled with replacement — the SAME resampled indices
    for every pair, because an opening's games are not independent across colours or pairs (every pair must have played the same
    openings) — drawn from numpy.random.default_rng(seed); a refit without a finite maximum counts as +/- 10000 Elo.
    Returns dict(elo [K], elo_lo [K], elo_hi [K], gamma [K], anchor, iterations, bootstrap, score = {pair: a's score},
    score_sd = {pair: standard deviation of a's score over the refits' resamples}). A rating is a statement about these players on
    these openings under these search settings, and nothing else."""
    K = int(results["n_players"])
    pairs = [tuple(p) for p in results["pairs"]]
    if not 0 <= int(anchor) < K:
        raise ValueError(f"ratings: anchor {anchor} is not one of the {K} players")
    P = [np.asarray(results["stats"][p]["pair_scores"], np.float64).ravel() for p in pairs]
    n_open = {p.size for p in P}
    if len(n_open) > 1:
        raise ValueError("ratings: every pair must have played the same openings")
    n_open = n_open.pop() if n_open else 0
    d = float(prior_draws)
    # the pairing graph must be connected
    comp = list(range(K))

    def find(x):
        while comp[x] != x:
            comp[x] = comp[comp[x]]
            x = comp[x]
        return x
    for a, b in pairs:
        if n_open > 0:
            comp[find(a)] = find(b)
    roots = {}
    for i in range(K):
        roots.setdefault(find(i), []).append(i)
    if len(roots) > 1:
        smallest = min(roots.values(), key=len)
        raise ValueError(f"ratings: the pairing graph is not connected: players {smallest} have played nobody outside their component")

    def totals(idx):
        """S [B, K], N [B, K, K], pair scores [B, pairs] for resampled opening indices idx [B, n_open]"""
        B = idx.shape[0]
        S = np.zeros((B, K)); N = np.zeros((B, K, K)); sc = np.zeros((B, len(pairs)))
        for j, (a, b) in enumerate(pairs):
            tot = 2.0 * P[j][idx].sum(axis=1)           # a's score over the 2 * n_open games
            S[:, a] += tot + d / 2; S[:, b] += 2.0 * n_open - tot + d / 2
            N[:, a, b] += 2.0 * n_open + d; N[:, b, a] += 2.0 * n_open + d
            sc[:, j] = tot / (2.0 * n_open)
        return S, N, sc

    S, N, sc = totals(np.arange(n_open)[None, :])
    if d == 0.0:
        for i in range(K):
            if S[0, i] == 0.0 or S[0, i] == N[0, i].sum():
                raise ValueError(f"ratings: player {i} scored {'nothing' if S[0, i] == 0.0 else 'every point'}: its rating has no finite "
                                 "maximum (prior_draws > 0 gives one)")
    g, iters = _bradley_terry(S, N)
    elo_of = lambda gam: 400.0 * (np.log10(gam) - np.log10(gam[:, anchor:anchor + 1]))  # noqa: E731
    point = elo_of(g)[0]
    out = dict(elo=point, gamma=g[0], anchor=int(anchor), iterations=iters, bootstrap=int(bootstrap),
               score={p: float(sc[0, j]) for j, p in enumerate(pairs)})
    if bootstrap and n_open > 0:
        rng = np.random.default_rng(seed)
        idx = rng.integers(0, n_open, size=(int(bootstrap), n_open))
        Sb, Nb, scb = totals(idx)
        gb, _ = _bradley_terry(Sb, Nb, tol=1e-10, max_iter=20000)
        with np.errstate(divide="ignore", invalid="ignore"):
            eb = elo_of(gb)
        eb = np.clip(np.nan_to_num(eb, nan=0.0, posinf=1e4, neginf=-1e4), -1e4, 1e4)
        out["elo_lo"], out["elo_hi"] = np.percentile(eb, 2.5, axis=0), np.percentile(eb, 97.5, axis=0)
        out["score_sd"] = {p: float(scb[:, j].std(ddof=1)) for j, p in enumerate(pairs)}
    else:
        out["elo_lo"], out["elo_hi"] = point.copy(), point.copy()
        out["score_sd"] = {p: float("nan") for p in pairs}
    return out


def host_match(engine, first, second, start_my, start_op):
    """match.play_match's loop for two network players, from given start positions instead of the empty board: per ply one
    engine.load_weights of the mover's blob (first.weights / second.weights), one engine.mcts_search over the live games and a numpy
    step. A player with an .arithmetic ("f32" / "f16x2") is searched in it: the engine is switched before that player's plies, and
    put back to the arithmetic it was in before returning. REPLACES the engine's network, as play_match does. Returns
    Engine.match_run's dict."""
    my = np.array(start_my, np.uint64).ravel(); op = np.array(start_op, np.uint64).ravel()
    n = int(my.size)
    alive = np.ones(n, bool)
    out = dict(rewards=np.zeros(n, np.float32), plies=np.zeros(n, np.int32), moves=np.full((n, 63), 255, np.uint8),
               final_bb=np.zeros((n, 2), np.uint64))
    own = engine.network_arithmetic()[0] if any(getattr(p, "arithmetic", None) for p in (first, second)) else None
    try:
        for ply in range(63):
            idx = np.nonzero(alive)[0]
            if idx.size == 0:
                break
            p = first if ply % 2 == 0 else second
            if own is not None:
                # (switched to f32 for the load: a load in f16x2 builds an image the next switch may throw away)
                engine.set_network_arithmetic("f32")
            engine.load_weights_conv(p.weights) if np.size(p.weights) == 12412 else engine.load_weights(p.weights)
            if own is not None:
                engine.set_network_arithmetic(getattr(p, "arithmetic", None) or own)
            res = engine.mcts_search(p.mcts_cfg, my[idx], op[idx], p.explores, action_selection=int(p.action))
            out["moves"][idx, ply] = res["best_action"]
            nmy, nop, over, w = match.step(my[idx], op[idx], res["best_action"])
            my[idx], op[idx] = nmy, nop
            out["plies"][idx] += 1
            first_moved = ply % 2 == 0
            out["rewards"][idx[over & w]] = 1.0 if first_moved else -1.0
            done = idx[over]
            # (after the move the mover's stones are `op`)
            out["final_bb"][done, 0] = op[done] if first_moved else my[done]
            out["final_bb"][done, 1] = my[done] if first_moved else op[done]
            alive[done] = False
    finally:
        if own is not None:
            engine.set_network_arithmetic(own)
    return out


# ---- agreement of two evaluations of one data set ---------------------------------------------------------------------------------------
def _first_argmax(x, allowed):
    """[n]: per row the first maximum of x [n][k] over the entries with allowed [n][k] (a later entry wins only when it compares greater);
    k for a row without an allowed entry"""
    n, k = x.shape
    best = np.full(n, k, np.int64)
    bv = np.zeros(n, np.float64)
    for c in range(k):
        take = allowed[:, c] & ((best == k) | (x[:, c] > bv))
        best = np.where(take, c, best)
        bv = np.where(take, x[:, c], bv)
    return best


def _masked_kl(a, b, allowed):
    """[n]: KL(softmax(a) || softmax(b)) with both softmaxes taken over the allowed entries only, in f64; 0 for a row without one"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        def logp(x):
            x = np.where(allowed, x, -np.inf)
            mx = np.max(x, axis=1, keepdims=True)
            mx = np.where(np.isfinite(mx), mx, 0.0)
            z = x - mx
            return z - np.log(np.sum(np.where(allowed, np.exp(z), 0.0), axis=1, keepdims=True))
        la, lb = logp(a), logp(b)
        term = np.where(allowed, np.exp(la) * (la - lb), 0.0)
    return np.sum(np.where(np.isfinite(term), term, 0.0), axis=1)


def dataset_agreement(rows_a, rows_b, my_bb, op_bb):
    """How far two evaluations of the same rows are apart: rows_a, rows_b = two `row_logits` arrays [n][12] of Engine.dataset_evaluate
    (say, arith="f32" and arith="f16x2") for the positions (my_bb, op_bb). Host code in f64 on downloaded rows. Returns a dict:
      rows               n
      max_abs_diff       max |a - b| over all twelve raw outputs;  mean_abs_diff: their mean
      pi_argmax_differs  the share of rows whose arg-max of the nine policy outputs over the LEGAL columns (top cell, bit 6 + 7 c of
                         my | op, free) differs; the first maximum wins, as in syn_dataset_evaluate's hits; a full column never counts
      v_argmax_differs   the same for the three value outputs
      mean_kl_pi         mean over rows of KL(softmax_a || softmax_b), both over the legal columns;  mean_kl_v: over the value triple
    A description of two arithmetics on one data set, not a statement about playing strength."""
    a = np.asarray(rows_a, np.float32).reshape(-1, 12).astype(np.float64)
    b = np.asarray(rows_b, np.float32).reshape(-1, 12).astype(np.float64)
    n = a.shape[0]
    if b.shape[0] != n:
        raise ValueError("rows_a and rows_b must have the same number of rows")
    occ = np.asarray(my_bb, np.uint64).ravel() | np.asarray(op_bb, np.uint64).ravel()
    if occ.size != n:
        raise ValueError("my_bb / op_bb must have one entry per row")
    if n == 0:
        return dict(rows=0, max_abs_diff=0.0, mean_abs_diff=0.0, pi_argmax_differs=0.0, v_argmax_differs=0.0, mean_kl_pi=0.0, mean_kl_v=0.0)
    legal = ((occ[:, None] >> (np.arange(9, dtype=np.uint64)[None, :] * _U(7) + _U(6))) & _U(1)) == 0
    every = np.ones((n, 3), bool)
    d = np.abs(a - b)
    return dict(rows=int(n), max_abs_diff=float(d.max()), mean_abs_diff=float(d.mean()),
                pi_argmax_differs=float(np.mean(_first_argmax(a[:, :9], legal) != _first_argmax(b[:, :9], legal))),
                v_argmax_differs=float(np.mean(_first_argmax(a[:, 9:], every) != _first_argmax(b[:, 9:], every))),
                mean_kl_pi=float(np.mean(_masked_kl(a[:, :9], b[:, :9], legal))),
                mean_kl_v=float(np.mean(_masked_kl(a[:, 9:], b[:, 9:], every))))
