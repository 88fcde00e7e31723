"""`python -m hanabi_sad_amd.eval_model`: the reference's pyhanabi/tools/eval_model.py -- score a published model (or a pair of
them) over fresh deals -- plus the measurement its result file models/op_raw_data.txt tabulates: `--cross_play` plays every
ordered pairing of a model pool over the same deals in ONE batched run (eval.cross_play) and prints the matrix in that file's
layout.

  --paper sad --weight a.pthw --num_player 2            self-play of one file (every seat the same weights)
  --paper op  --method sad --idx1 0 --idx2 3            one cell: M0 on seat 0 with M3 on seat 1
  --paper obl --obl_path obl.pthw                       self-play of an OBL model
  --paper op  --method sad --idx 0 3 6 9 --cross_play   the 4 x 4 matrix
  --paper sad --weight a.pthw b.pthw c.pthw --cross_play
  --paper op  --method sad --idx 0 3 --cross_play --bots cautious piers    the matrix with rule-bot partners (rulebot.PRESETS)
  ... --cross_play --bots piers --behaviour             the matrix, then per pairing and seat the behaviour counters and rates
  ... --save_games g.jsonl --save_games_where "score<=10,flag=last_life,seat=1"    also write the games the filter keeps to a file
                                                        (game_record; read it with python -m hanabi_sad_amd.game_record g.jsonl)
  --paper op  --method sad --idx 0 --search_worlds 8    M0 in self-play, blueprint only and blueprint + search over the same deals
  ... --search_worlds 32 --search_rounds 8,8,16         the same with the search in rounds (paired statistics, pruning)
  ... --search_worlds 8 --search_depth 2                the same with every world stopped 2 moves after the candidate action and
                                                        valued as score so far + the blueprint's Q
  ... --search_worlds 8 --search_sampler learned --search_belief belief.pthw    the worlds' hands drawn from a learned belief head
                                                        (python -m hanabi_sad_amd.belief fits one)

As in the reference the deals are seeds 1 .. num_game * num_run, bombing out keeps the score (bomb 0) and everyone acts greedily.
Whether the env appends SAD's greedy-action section is read off the models' input width (838 vs 783 features in the 2-player
game)."""
import argparse
import os

from .eval import cross_play, env_dims, format_behaviour_table, format_cross_play_table, play_seatings
from .rulebot import PRESETS


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m hanabi_sad_amd.eval_model")
    p.add_argument("--paper", default="sad", type=str, choices=["sad", "op", "obl"])
    p.add_argument("--num_game", default=5000, type=int)
    p.add_argument("--num_run", default=1, type=int, help="total num game = num_game * num_run")
    p.add_argument("--weight", default=None, type=str, nargs="+", help="--paper sad: the weight file (several with --cross_play)")
    p.add_argument("--num_player", default=None, type=int)
    p.add_argument("--method", default="sad-aux-op", type=str, help="sad-aux-op/sad-aux/sad-op/sad")
    p.add_argument("--idx1", default=1, type=int, help="which model to use?")
    p.add_argument("--idx2", default=1, type=int)
    p.add_argument("--device", default="cuda:0", type=str)
    p.add_argument("--obl_path", default=None, type=str)
    p.add_argument("--cross_play", action="store_true", help="print the score matrix of the pool (--idx / several --weight)")
    p.add_argument("--idx", default=None, type=int, nargs="+", help="--paper op --cross_play: the zoo models of the pool")
    p.add_argument("--bots", default=[], type=str, nargs="+", choices=sorted(PRESETS),
                   help="--cross_play: rule-bot presets appended to the pool (hand-coded partners; rulebot.PRESETS)")
    p.add_argument("--behaviour", action="store_true", help="--cross_play: after the matrix, one line per (pairing, seat) with the "
                   "behaviour counters of the moves made there and their rates (eval.BehaviourStats; include/hsad.h, HSAD_BH_*)")
    p.add_argument("--save_games", default=None, type=str, metavar="FILE", help="record the games on the device and write them to FILE "
                   "as JSON lines (game_record.save): every finished game, or those --save_games_where keeps")
    p.add_argument("--save_games_where", default=None, type=str, metavar="FILTER", help="with --save_games: comma-separated terms "
                   "score / moves (<=, >=, =), lives<=K, end=lives|deck|perfect, flag=NAME, seat=P (game_record.GameFilter.parse), "
                   "e.g. \"score<=10,flag=last_life,seat=1\"")
    p.add_argument("--temperature", default=None, type=float, nargs="+", metavar="T", help="the models play their softmax policy: moves "
                   "sampled from the softmax over the legal advantages at this temperature (one value, or one per model; 0 = greedy; "
                   "bf16 models only; --bots ignore it)")
    p.add_argument("--sample_seed", default=0, type=int, help="with --temperature: seeds the sample draws")
    p.add_argument("--root", default=None, type=str, help="folder that holds models/op/<method>/M{idx}.pthw (default: the repository)")
    p.add_argument("--precision", default="bf16", type=str, choices=["bf16", "fp32"])
    p.add_argument("--search_worlds", default=0, type=int, help="> 0 with a single --idx: also play with blueprint-policy search "
                   "(search.play_with_search), this many sampled worlds per legal action")
    p.add_argument("--search_threshold", default=0.05, type=float, help="deviate from the blueprint only for a larger value gain")
    p.add_argument("--search_replay", default=0, type=int, help="1: rebuild every sampled world's LSTM states by replaying the game's "
                   "history (play_with_search(replay_history=True))")
    p.add_argument("--search_consistent", default=0, type=int, help="1 (with --search_replay 1): count only the worlds in which the "
                   "blueprint shows the partners' observed greedy actions")
    p.add_argument("--search_seat", default=None, type=int, help="the one seat that searches (default: every seat)")
    p.add_argument("--search_sampler", default="rejection", type=str, choices=["rejection", "stratified", "learned"],
                   help="how the sampled worlds' hidden hands are drawn: hsad_env_determinize, hsad_env_determinize_exact with the "
                   "worlds of a game stratified over its exact belief, or (with --search_belief) hsad_env_determinize_belief_worlds under "
                   "a learned belief head")
    p.add_argument("--search_belief", default=None, type=str, metavar="FILE", help="with --search_sampler learned: the saved belief head "
                   "(belief.BeliefHead.save; python -m hanabi_sad_amd.belief writes belief.pthw)")
    p.add_argument("--search_rounds", default=None, type=lambda s: tuple(int(x) for x in s.split(",")),
                   help="world counts per round, e.g. 8,8,16 (their sum must be --search_worlds): search in rounds, dropping hopeless "
                   "actions in between, and choose by the paired statistics (search.choose_action_paired)")
    p.add_argument("--search_prune_z", default=2.0, type=float, help="with --search_rounds: drop an action whose paired mean lies more "
                   "than this many paired standard errors below the round's leader")
    p.add_argument("--search_deviate_z", default=0.0, type=float, help="with --search_rounds: deviate only where the paired gain over "
                   "the blueprint's action also exceeds this many of its standard errors")
    p.add_argument("--search_depth", default=None, type=int, metavar="D", help="with --search_worlds: stop every sampled world D moves "
                   "after the candidate action and value it as its score so far + the blueprint's own Q "
                   "(play_with_search(depth=D)); not with --search_rounds")
    p.add_argument("--search_horizon_value", default="mover", type=str, choices=["mover", "team"],
                   help="with --search_depth: the Q of the seat on turn at the horizon, or the sum over the game's seats")
    return p.parse_args(argv)


def check_search_depth(args):
    """the usage errors of --search_depth; touches no device"""
    if args.search_depth is None:
        return
    if args.search_worlds < 1:
        raise SystemExit("--search_depth needs --search_worlds N > 0")
    if args.search_rounds is not None:
        raise SystemExit("--search_depth and --search_rounds do not combine (the round kernel compares whole scores)")
    if args.search_depth < 0:
        raise SystemExit("--search_depth must not be negative")


def load_pool(args):
    """-> (agents, names, title, players)"""
    from .checkpoint import agent_from_file, load_op_model
    if args.paper == "sad":
        files = args.weight or []
        if not files or not all(os.path.exists(f) for f in files):
            raise SystemExit("--paper sad needs --weight FILE (existing file%s)" % ("s" if args.cross_play else ""))
        if not args.cross_play and len(files) != 1:
            raise SystemExit("several --weight files need --cross_play")
        agents = [agent_from_file(f, args.device, 3, 0.999, args.precision) for f in files]
        return agents, ["W%d" % i for i in range(len(files))], "SAD", args.num_player or 2
    if args.paper == "op":
        idx = args.idx if args.cross_play else [args.idx1, args.idx2]
        if not idx:
            raise SystemExit("--paper op --cross_play needs --idx I J K ...")
        agents = [load_op_model(args.method, i, None, args.device, root=args.root, precision=args.precision)[0] for i in idx]
        return agents, ["M%d" % i for i in idx], args.method.upper(), 2
    from .obl import load_obl_model
    if not args.obl_path or not os.path.exists(args.obl_path):
        raise SystemExit("--paper obl needs --obl_path FILE")
    return [load_obl_model(args.obl_path, args.device, args.precision)], ["OBL"], "OBL", 2


def load_search_belief(args):
    """--search_sampler learned --search_belief FILE -> the head's state dict (None for the other samplers); a usage error when one is
    given without the other, when the file is missing or when it holds no belief head.  Touches no device."""
    if (args.search_sampler == "learned") != (args.search_belief is not None):
        raise SystemExit("--search_sampler learned and --search_belief FILE go together")
    if args.search_belief is None:
        return None
    if not os.path.isfile(args.search_belief):
        raise SystemExit("--search_belief %s: no such file" % args.search_belief)
    import torch
    from .belief import check_state
    try:
        sd = torch.load(args.search_belief, map_location="cpu")
        if not isinstance(sd, dict):
            raise ValueError("not a belief head: the file holds a %s" % type(sd).__name__)
        check_state(sd)
    except ValueError as e:
        raise SystemExit("--search_belief %s: %s" % (args.search_belief, e))
    except Exception as e:      # not a torch file at all
        raise SystemExit("--search_belief %s: not a saved belief head (%s)" % (args.search_belief, type(e).__name__))
    return sd


def search_report(args):
    """--search_worlds N with a single --idx: the model in self-play over the deals 1 .. num_game * num_run, blueprint only and
    blueprint + search -> (SearchPlay without search, SearchPlay with it)"""
    from .checkpoint import load_op_model
    from .search import play_with_search
    if args.paper != "op" or args.cross_play or not args.idx or len(args.idx) != 1:
        raise SystemExit("--search_worlds needs --paper op and a single --idx I (no --cross_play)")
    belief = load_search_belief(args)
    agent = load_op_model(args.method, args.idx[0], None, args.device, root=args.root, precision=args.precision)[0]
    sad = getattr(agent.online, "F", None) == env_dims(2, 5, sad=True)[0]
    n = args.num_game * args.num_run
    kw = dict(precision=args.precision, device=args.device, threshold=args.search_threshold,
              searcher="all" if args.search_seat is None else args.search_seat)
    base = play_with_search(agent, n, 1, 0, sad, worlds=0, **kw)
    if args.search_rounds is not None:
        kw.update(rounds=args.search_rounds, prune_z=args.search_prune_z, deviate_z=args.search_deviate_z)
    if args.search_depth is not None:
        kw.update(depth=args.search_depth, horizon_value=args.search_horizon_value)
    res = play_with_search(agent, n, 1, 0, sad, worlds=args.search_worlds, replay_history=bool(args.search_replay),
                           consistent_only=bool(args.search_consistent), sampler=args.search_sampler, belief=belief, **kw)
    print("blueprint: %f +/- %f" % (base.mean, base.sem), "; perfect: ", base.perfect)
    line = "; deviations per game: %f" % float(res.deviations.double().mean())
    if args.search_depth is not None:
        line += " ; depth %d (%s): %f of the worlds cut at the horizon" % (args.search_depth, args.search_horizon_value, res.cut_share)
    print("blueprint + search (%d worlds): %f +/- %f" % (args.search_worlds, res.mean, res.sem), "; perfect: ", res.perfect, line)
    return base, res


def main(argv=None):
    args = parse_args(argv)
    if args.behaviour and not args.cross_play:
        raise SystemExit("--behaviour needs --cross_play (the table has one line per pairing of the matrix and seat)")
    if args.save_games_where and not args.save_games:
        raise SystemExit("--save_games_where needs --save_games FILE")
    where = None
    if args.save_games:
        from .game_record import GameFilter, save
        try:
            where = GameFilter.parse(args.save_games_where) if args.save_games_where else True
        except ValueError as e:
            raise SystemExit("--save_games_where: %s" % e)
    if args.temperature is not None and any(not t >= 0 or t == float("inf") for t in args.temperature):
        raise SystemExit("--temperature must be finite and not negative")
    load_search_belief(args)      # the usage errors, before anything is loaded
    check_search_depth(args)
    if args.search_worlds > 0:
        if args.temperature is not None:
            raise SystemExit("--temperature samples tournament seats (no --search_worlds: the search plays the blueprint's greedy moves)")
        if args.save_games:
            raise SystemExit("--save_games records tournament games (no --search_worlds)")
        return search_report(args)
    agents, names, title, P = load_pool(args)
    net = agents[0].online
    n, kw = args.num_game * args.num_run, dict(precision=args.precision, device=args.device, hand_size=5 if P <= 3 else 4)
    sad = args.paper == "obl" or getattr(net, "F", None) == env_dims(P, kw["hand_size"], sad=True)[0]
    if args.bots and not args.cross_play:
        raise SystemExit("--bots needs --cross_play (the bots join the pool of the matrix)")
    if args.temperature is not None:
        if len(args.temperature) not in (1, len(agents)):
            raise SystemExit("--temperature takes one value or one per model (%d); got %d" % (len(agents), len(args.temperature)))
        temps = list(args.temperature) * (len(agents) if len(args.temperature) == 1 else 1)
        kw.update(temperature=temps + [0.0] * (len(args.bots) if args.cross_play else 0), sample_seed=args.sample_seed)
    if args.cross_play:
        agents, names = agents + [PRESETS[b] for b in args.bots], names + list(args.bots)
        if P != 2:
            raise SystemExit("--cross_play is the two-player matrix")
        if args.behaviour:
            kw["behaviour"] = True
        if where is not None:
            kw.update(records=where, names=names)
        res = cross_play(agents, n, 1, 0, sad, **kw)
        if where is not None:
            save(args.save_games, res.records)
            print("%d game(s) written to %s" % (len(res.records), args.save_games))
        print(format_cross_play_table("self-play & cross-play of %s" % title, names, res.mean, res.row_mean))
        if args.behaviour:
            print()
            print(format_behaviour_table(names, res.behaviour))
        return res
    seating = [0] * P if len(agents) == 1 else list(range(P))
    if where is not None:
        kw.update(records=where, names=names)
    res = play_seatings(agents, [seating], n, 1, 0, sad, **kw)
    print("score: %f +/- %f" % (res.mean[0], res.sem[0]), "; perfect: ", res.perfect[0])
    if where is not None:
        save(args.save_games, res.records)
        print("%d game(s) written to %s" % (len(res.records), args.save_games))
    return res


if __name__ == "__main__":
    main()
