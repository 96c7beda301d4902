"""Value-greedy play on VecNardeEnv: the TD-Gammon way to choose a move.

A TD-Gammon agent (the reference's README: the 198-float Tesauro encoding,
README.md:42-102, reward "+1 if WHITE wins") does not score action codes: it
scores the positions a roll can lead to -- the afterstates -- with a value
network and plays the best one.  ValuePlayer does that for B envs at once,
everything on the device: VecNardeEnv.afterstates() expands the roll,
`net` scores the rows, VecNardeEnv.pick_afterstate() chooses, step() plays.
On a rules="full4" env the rows are whole turns (turn_afterstates(),
pick_turn()): four sub-moves on doubles, the max-dice-used rule.
With a value_net.ValueMLP the rows are scored inside the expansion
(scored_afterstates() / scored_turn_afterstates(): one float a row, the
198-float rows never made).  plies=2 searches one ply deeper
(lookahead_afterstates(): each row's value is the expectation, over the
opponent's rolls, of the opponent's best reply under the same net);
LookaheadPlayer is that search for either rule set
(lookahead_turn_afterstates() on a rules="full4" env); with top=k it searches
only each env's k best rows by one-ply value (top_rows(),
VecNardeEnv.lookahead_records(), pick_slots()).
play_match() answers "is net A better than net B, or than random play?":
whole games in one launch a colour assignment (VecNardeEnv.value_rollout());
play_turn_match() is the same on a rules="full4" env
(VecNardeEnv.turn_value_rollout()).
play_league() ranks N nets, random play included, by a whole round-robin in
one launch (VecNardeEnv.value_rollout_league() /
turn_value_rollout_league(): a net per env and colour from a table).
"""


def _is_mlp(net):
    """net quacks like a value_net.ValueMLP (struct() and pack())."""
    return hasattr(net, "struct") and hasattr(net, "pack")


class ValuePlayer:
    """net: a callable (R,198) float32 -> (R,) or (R,1) values (a
    torch.nn.Module on the env's device).  perspective "white": the values
    are white's (the README's reward) -- white plays the largest, black the
    smallest; "mover": they are the side's that has just moved -- always the
    largest.
    fused: None -- the scored expansion when net is a value_net.ValueMLP;
    False -- never (every step as with any other module); True -- required
    (a TypeError for another module).  cap: the rows every step's arrays
    hold (fused only); with it a step makes no synchronise, and rows past
    cap are not played.  plies: 1 -- the rows' own values; 2 -- their
    two-ply values (the fused path, perspective "white", rules="ref2")."""

    def __init__(self, env, net, perspective="white", fused=None, cap=None, plies=1):
        from .vector import PERSPECTIVES

        if perspective not in PERSPECTIVES:
            raise ValueError(f"perspective must be one of {tuple(PERSPECTIVES)}")
        self.env, self.net, self.perspective = env, net, perspective
        self._expand, self._pick = env._twin("afterstates"), env._twin("pick_afterstate")
        is_mlp = _is_mlp(net)
        if fused and not is_mlp:
            raise TypeError("fused=True needs a gym_narde.value_net.ValueMLP")
        self.fused = is_mlp if fused is None else bool(fused)
        if cap is not None and not self.fused:
            raise ValueError("cap is the fused path's")
        self.cap = None if cap is None else int(cap)
        self._scored = env._twin("scored_afterstates")
        if plies not in (1, 2):
            raise ValueError("plies must be 1 or 2")
        if plies == 2:
            if not is_mlp:
                raise TypeError("plies=2 needs a gym_narde.value_net.ValueMLP")
            if not self.fused:
                raise ValueError("plies=2 is the fused path's")
            if perspective != "white":
                raise ValueError('plies=2 needs perspective "white"')
            if env.full:
                raise ValueError('plies=2 is rules="ref2" only')
        self.plies = plies
        self._lookahead = env._twin("lookahead_afterstates")

    def values(self, aft):
        """net(feat), with the rows that end the game set to their known
        outcome: the step's reward (1, or 2 when the loser has borne off
        nothing) for the side that made the move -- negated in white's
        perspective when that side is black."""
        t = self.env.torch
        if aft.cap == 0:
            return t.empty(0, dtype=t.float32, device=self.env.device)
        with t.no_grad():
            v = self.net(aft.feat).reshape(-1).to(t.float32)
        outcome = aft.reward.to(t.float32)
        if self.perspective == "white":
            # after a terminal step the mover is not flipped: the row's player
            # one-hot (columns 196 white, 197 black) names the winner
            outcome = t.where(aft.feat[:, 197] > 0.5, -outcome, outcome)
        return t.where(aft.reward != 0, outcome, v)

    def step(self, epsilon=None, tag=None, seed=0):
        """One ply for every env: the next step's dice, their afterstates, the
        values, the pick, the step.  Returns (obs, reward, terminated,
        truncated, info, aft, values, actions); an env with no expressible
        play steps with (0, 0), which moves nothing (rules="full4": actions
        are (B,4,2) plays, all -1 for an env that has to pass).  On the fused
        path aft.feat is None."""
        env = self.env
        dice = env.dice()
        if self.plies == 2:
            aft, values = self._lookahead(self.net, dice, cap=self.cap)
        elif self.fused:
            aft, values = self._scored(self.net, dice, cap=self.cap, perspective=self.perspective)
        else:
            aft = self._expand(dice)
            values = self.values(aft)
        actions, row = self._pick(aft, values, self.perspective, epsilon, tag, seed)
        obs, reward, terminated, truncated, info = env.step(actions)
        info = dict(info, dice=dice, row=row)
        return obs, reward, terminated, truncated, info, aft, values, actions


class LookaheadPlayer(ValuePlayer):
    """The two-ply player for either rule set: every row valued by the mean,
    over the opponent's rolls, of the opponent's best reply under net (a
    value_net.ValueMLP) -- lookahead_afterstates() on a rules="ref2" env,
    lookahead_turn_afterstates() on a rules="full4" one.  The fused path,
    perspective "white"; cap and step() as ValuePlayer's.
    top: None -- every row is searched.  top = k (1 .. NARDE_TOPK_MAX) -- the
    pruned search: only each env's k best rows by
    one-ply value are searched, and the best of those by two-ply value is
    played.  Five device calls a ply with static shapes: recorded_afterstates()
    / recorded_turn_afterstates(), top_rows(k, records), lookahead_records()
    of the roots, pick_slots(), step().  step() then returns the same tuple --
    values the rows' one-ply values -- with sel and score (the slots' two-ply
    scores) in info.  top = 1 plays exactly ValuePlayer's moves."""

    def __init__(self, env, net, cap=None, top=None):
        from . import _lib

        if not _is_mlp(net):
            raise TypeError("LookaheadPlayer needs a gym_narde.value_net.ValueMLP")
        super().__init__(env, net, perspective="white", fused=True, cap=cap, plies=1)
        self.plies = 2
        if top is not None:
            if isinstance(top, bool) or not isinstance(top, int):
                raise TypeError("top must be None or an int")
            if not 1 <= top <= _lib.TOPK_MAX:
                raise ValueError(f"top must be in 1 .. {_lib.TOPK_MAX}")
        self.top = top
        self._recorded = env._twin("recorded_afterstates")

    def step(self, epsilon=None, tag=None, seed=0):
        if self.top is None:
            return super().step(epsilon, tag, seed)
        if epsilon is not None or tag is not None:
            raise ValueError("the pruned search (top) plays greedily: no epsilon")
        env = self.env
        dice = env.dice()
        aft, values, records = self._recorded(self.net, dice, cap=self.cap)
        sel, roots = env.top_rows(aft, values, self.top, records)
        two = env.lookahead_records(roots, self.net)
        actions, row, score = env.pick_slots(aft, values, sel, two.view(env.num_envs, self.top))
        obs, reward, terminated, truncated, info = env.step(actions)
        info = dict(info, dice=dice, row=row, sel=sel, score=score)
        return obs, reward, terminated, truncated, info, aft, values, actions


class PlayoutPlayer:
    """Playout-greedy play for either rule set: every
    ply, each env's k best rows by one-ply value under net (a
    value_net.ValueMLP) are played out `trials` times to the end --
    max_plies plies at most -- under playout_net (default: net, for both
    colours), and the candidate with the best mean outcome is played.  Five
    device calls a ply: recorded_afterstates() / recorded_turn_afterstates(),
    top_rows(), playout(), pick_playout(), step().
    common_dice: trial j of every root meets the same dice -- across the envs
    as well as across one env's candidates (one id per trial for the whole
    call), which is what makes an env's candidates comparable; False gives
    every trial of every root a stream of its own.  truncated: an unfinished
    trial counts at playout_net's value of the position it stopped at (the mean
    over all trials) instead of being left out.  The playouts' seed of a ply
    is `seed` plus the env's ply counter, so plies differ; the counter is read
    when the player is made and advanced by step() (plies stepped by others
    in between: sync_ply()).  cap: the rows every ply's arrays hold; with it
    a ply makes no synchronise, and rows past cap are not played.  k = 1
    plays exactly ValuePlayer's moves."""

    def __init__(self, env, net, k=4, trials=64, max_plies=400, playout_net=None, common_dice=True, truncated=False,
                 cap=None, seed=0):
        if not _is_mlp(net):
            raise TypeError("PlayoutPlayer needs a gym_narde.value_net.ValueMLP")
        self.env, self.net = env, net
        self.playout_net = net if playout_net is None else playout_net
        self.k, self.trials, self.max_plies = int(k), int(trials), int(max_plies)
        self.common_dice, self.truncated = bool(common_dice), bool(truncated)
        self.cap = None if cap is None else int(cap)
        self.seed = int(seed)
        self._recorded = env._twin("recorded_afterstates")
        self.sync_ply()

    def sync_ply(self):
        """Read the env's ply counter again (one synchronise)."""
        self._ply = self.env.ply

    def step(self):
        """One ply for every env.  Returns what ValuePlayer.step() returns --
        (obs, reward, terminated, truncated, info, aft, values, actions) --
        with sel, score and the PlayoutResult (playout) in info besides dice
        and row."""
        env = self.env
        dice = env.dice()
        aft, values, records = self._recorded(self.net, dice, cap=self.cap)
        sel, roots = env.top_rows(aft, values, self.k, records)
        res = env.playout(roots, self.trials, self.playout_net, max_plies=self.max_plies,
                          seed=(self.seed + self._ply) & (2 ** 64 - 1), common_dice=self.common_dice,
                          leaf=self.truncated)
        actions, row, score = env.pick_playout(aft, values, sel, res, leaf=self.truncated)
        obs, reward, terminated, truncated, info = env.step(actions)
        self._ply = (self._ply + 1) & 0xFFFFFFFF
        info = dict(info, dice=dice, row=row, sel=sel, score=score, playout=res)
        return obs, reward, terminated, truncated, info, aft, values, actions


def play_match(env, net_a, net_b, plies, epsilon=None, seed=0):
    """net_a against net_b (value_net.ValueMLPs on the env's device; net_b
    None: the random-legal policy, the baseline) on a rules="ref2" env, every
    env playing with both colour assignments: env.reset() and one
    value_rollout() launch of `plies` plies with a as white and b as black,
    then env.reset() and one with the colours swapped.  Games that finish
    inside a launch count, those still running at its end do not; envs
    auto-reset, so one env plays several games.  A game the TimeLimit
    truncates counts as a game and gives neither side points.  epsilon: both
    sides explore with it (ply k of either launch under the tag k).
    Returns {"games", "points_a", "points_b", "by_colour"}: the totals over
    both launches, and by_colour = {"a_white": {"games", "points_a",
    "points_b"}, "a_black": {...}} from env.stats() after each launch."""
    if env.full:
        raise ValueError('play_match() is rules="ref2" only')
    return _match(env, net_a, net_b, plies, epsilon, seed)


def play_turn_match(env, net_a, net_b, plies, epsilon=None, seed=0):
    """play_match() on a rules="full4" env: whole turns, one
    turn_value_rollout() launch of `plies` plies per colour assignment
    (DESIGN.md section 20).  The same arguments and the same dictionary."""
    if not env.full:
        raise ValueError('play_turn_match() is rules="full4" only')
    return _match(env, net_a, net_b, plies, epsilon, seed)


def _match(env, net_a, net_b, plies, epsilon, seed):
    if net_a is None:
        raise ValueError("net_a is the net under test; pass None as net_b for the random baseline")
    by = {}
    bufs = env._twin("value_rollout_buffers")(plies, *[False] * 6)  # every per-ply output off
    rollout = env._twin("value_rollout")
    tag = None if epsilon is None else 0
    for name, white, black in (("a_white", net_a, net_b), ("a_black", net_b, net_a)):
        env.reset()
        rollout(plies, white, black, epsilon=epsilon, tag=tag, seed=seed, bufs=bufs)
        games, pw, pb = (int(x) for x in env.stats().sum(0).tolist())
        pa, pbb = (pw, pb) if name == "a_white" else (pb, pw)
        by[name] = {"games": games, "points_a": pa, "points_b": pbb}
    return {"games": sum(v["games"] for v in by.values()), "points_a": sum(v["points_a"] for v in by.values()),
            "points_b": sum(v["points_b"] for v in by.values()), "by_colour": by}


def playout_values(env, roots, net, trials, max_plies=1000, seed=0, id_base=0, common_dice=False, truncated=False):
    """What the positions `roots` are worth to white when both colours play
    value-greedy under `net` to the end: env.playout() with one net, reduced to
    (mean, stderr), float64 device tensors of one entry a root (DESIGN.md
    section 22).  roots: (N, 8) int32 records or a get_state()-style dict.
    truncated: count a trial max_plies cut short at the net's value of the
    position it stopped at (mean over all trials) instead of leaving it out."""
    res = env.playout(roots, trials, net, max_plies=max_plies, seed=seed, id_base=id_base, common_dice=common_dice,
                      leaf=truncated)
    return res.mean(truncated=truncated), res.stderr()


def league_pairs(n, random=False, self_play=False):
    """The ordered pairs (white, black) of a round-robin over nets 0 .. n - 1:
    every i != j, white-major; random: index -1 -- the random-legal policy --
    joins as one more participant, last; self_play: (i, i) for every net too
    (in its place of the white-major order)."""
    n = int(n)
    if n < 1:
        raise ValueError("n must be >= 1")
    who = list(range(n)) + ([-1] if random else [])
    return [(w, b) for w in who for b in who if w != b or (self_play and w >= 0)]


def league_result(stats, white, black, n, random=False):
    """A league launch's per-env statistics as pairing matrices: pure host
    arithmetic.  stats: (B, 3) integers, env.stats()'s (games, white's points,
    black's points); white, black: the (B,) indices the launch was given; n:
    the number of nets.  An index outside 0 .. n - 1 is the random participant
    (random=True: it is the matrices' last row and column; otherwise a
    ValueError).
    Returns a dict: games, points_white, points_black -- int64 (P, P), indexed
    [white][black], P = n + random --; margin (P, P) float64, margin[i][j] =
    i's points a game over j with both colour assignments pooled, NaN where
    the two played no game (margin[i][j] == -margin[j][i]); stderr_bound (P,
    P), 2 / sqrt(the pooled games): a game gives a side 0, 1 or 2 points, so
    that bounds the margin's standard error; score (P,), the mean of row i of
    margin over the opponents i has games against (NaN with none)."""
    import numpy as np

    stats = np.asarray(stats, dtype=np.int64)
    white = np.asarray(white, dtype=np.int64).reshape(-1)
    black = np.asarray(black, dtype=np.int64).reshape(-1)
    n = int(n)
    if stats.ndim != 2 or stats.shape[1] != 3 or white.shape[0] != stats.shape[0] or black.shape[0] != stats.shape[0]:
        raise ValueError("stats must be (B, 3), white and black (B,)")
    P = n + (1 if random else 0)
    wi = np.where((white >= 0) & (white < n), white, n)
    bi = np.where((black >= 0) & (black < n), black, n)
    if not random and ((wi == n).any() or (bi == n).any()):
        raise ValueError("an index outside 0 .. n - 1 is the random participant: pass random=True")
    out = {}
    for k, name in enumerate(("games", "points_white", "points_black")):
        m = np.zeros((P, P), dtype=np.int64)
        np.add.at(m, (wi, bi), stats[:, k])
        out[name] = m
    g, pw, pb = out["games"], out["points_white"], out["points_black"]
    pooled = (g + g.T).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["margin"] = np.where(pooled > 0, (pw + pb.T - pb - pw.T) / pooled, np.nan)
        out["stderr_bound"] = np.where(pooled > 0, 2.0 / np.sqrt(pooled), np.nan)
    score = np.full(P, np.nan)
    for i in range(P):
        has = (pooled[i] > 0) & (np.arange(P) != i)
        if has.any():
            score[i] = out["margin"][i][has].mean()
    out["score"] = score
    return out


def play_league(env, nets, plies, random=False, self_play=False, epsilon=None, seed=0, pairs=None):
    """A whole round-robin in one launch, on either rule set (DESIGN.md
    section 27): env e plays the pair e mod len(pairs) of league_pairs(len(nets),
    random, self_play) -- or of `pairs`, a list of (white, black) indices into
    nets, -1 the random-legal policy -- as (white, black) for every game it
    plays.  env.reset(), one value_rollout_league() / turn_value_rollout_league()
    launch of `plies` plies with every per-ply output off, then
    league_result(env.stats(), ...).  Games still running at the launch's end
    do not count, and a game the TimeLimit truncates counts as a game and gives
    neither side points: play_match()'s rules.  epsilon: every side explores
    with it (ply k under the tag k).  nets: 1 .. 64 value_net.ValueMLPs on the
    env's device.  Returns league_result()'s dict with "pairs", "white" and
    "black" (the host lists used) added."""
    import numpy as np

    from . import _lib

    nets = list(nets)
    if not 1 <= len(nets) <= _lib.LEAGUE_NETS_MAX:
        raise ValueError(f"a league has 1 .. {_lib.LEAGUE_NETS_MAX} nets, not {len(nets)}")
    for i, net in enumerate(nets):
        if not (hasattr(net, "struct") and hasattr(net, "l1")):
            raise TypeError(f"nets[{i}] must be a gym_narde.value_net.ValueMLP")
        if net.l1.weight.device != env.device:
            raise ValueError(f"nets[{i}] must live on the env's device")
    if pairs is None:
        pairs = league_pairs(len(nets), random, self_play)
    pairs = [(int(w), int(b)) for w, b in pairs]
    if not pairs:
        raise ValueError("no pairs to play")
    if any(not 0 <= x < len(nets) for p in pairs for x in p):
        random = True  # (a given pair names the random participant)
    B = env.num_envs
    if B < len(pairs):
        raise ValueError(f"{B} envs cannot hold {len(pairs)} pairs: every pair needs an env")
    t = env.torch
    idx = np.arange(B) % len(pairs)
    white = np.asarray([p[0] for p in pairs], dtype=np.int32)[idx]
    black = np.asarray([p[1] for p in pairs], dtype=np.int32)[idx]
    table = env.net_table(nets)
    bufs = env._twin("value_rollout_buffers")(plies, *[False] * 6)  # every per-ply output off
    rollout = env._twin("value_rollout_league")
    env.reset()
    rollout(plies, table, t.as_tensor(white, device=env.device), t.as_tensor(black, device=env.device),
            epsilon=epsilon, tag=None if epsilon is None else 0, seed=seed, bufs=bufs)
    res = league_result(env.stats().cpu().numpy(), white, black, len(nets), random=random)
    res.update(pairs=pairs, white=white, black=black)
    return res
