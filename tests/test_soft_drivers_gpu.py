"""GPU: the command lines of softmax-policy acting, each once on Hanabi-Small (2 colours, hands of 2, 3 information tokens, 1 life):
`clone --teacher FILE --teacher_temperature T --eval_temperature T` and `selfplay --partner FILE --partner_temperature T`; and, in the
standard game (eval_model takes no rule flags), `eval_model --weight FILE [FILE --cross_play --bots piers] --temperature T [T]
--save_games FILE` on files of the default architecture."""
import re

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
DEV = "cuda:0"
SMALL = ["--hand_size", "2", "--colors", "2", "--max_information_tokens", "3", "--max_life_tokens", "1"]
RULES = dict(colors=2, ranks=5, max_information_tokens=3, max_life_tokens=1)


@pytest.fixture(scope="module")
def teacher_file(tmp_path_factory):
    from hanabi_sad_amd.eval import env_dims
    from hanabi_sad_amd.selfplay import init_weights
    F, A = env_dims(2, 2, True, **RULES)
    f = str(tmp_path_factory.mktemp("soft") / "teacher.pthw")
    torch.save(init_weights(F, 64, A, 2, 31), f)
    return f


def test_clone_driver_samples_its_teacher_and_scores_the_sampled_clone(teacher_file, tmp_path, capsys):
    from hanabi_sad_amd import clone, game_record as gr
    argv = ["--teacher", teacher_file, "--num_game", "64", "--num_epoch", "2", "--sad", "1", "--max_len", "40", "--batchsize", "16",
            "--rnn_hid_dim", "64", "--num_eval_game", "32", "--save_dir", str(tmp_path), "--train_device", DEV, "--teacher_temperature", "1",
            "--eval_temperature", "1"] + SMALL
    assert clone.main(argv) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("epoch ")]
    assert len(lines) == 2
    for ln in lines:
        m = re.search(r"self-play score ([0-9.]+) \(sampled at temperature 1: ([0-9.]+)\)", ln)
        assert m and 0.0 <= float(m.group(1)) <= 10.0 and 0.0 <= float(m.group(2)) <= 10.0, ln
    # the games that were cloned are the teacher's sampled games: some move is not the greedy one
    records = gr.load(str(tmp_path / "games.jsonl"))
    assert len(records) == 64 and any(r.moves != r.greedy for r in records)


def test_selfplay_driver_trains_next_to_a_warm_partner(teacher_file, capsys):
    from hanabi_sad_amd import selfplay
    selfplay.main(["--num_game", "128", "--partner", teacher_file, "--partner_temperature", "1", "--num_update", "3", "--burn_in_frames", "64",
                   "--replay_buffer_size", "512", "--batchsize", "32", "--rnn_hid_dim", "64"] + SMALL)
    out = capsys.readouterr().out
    loss = re.findall(r"update 0 loss (\S+) grad_norm (\S+)", out)
    assert loss and np.isfinite(float(loss[0][0])) and np.isfinite(float(loss[0][1])), out[-2000:]
    lines = re.findall(r"^partner (\S+): score (\S+) \(", out, flags=re.M)
    assert [n for n, _ in lines] == ["teacher.pthw"] and 0.0 <= float(lines[0][1]) <= 10.0, out[-2000:]


def test_eval_model_command_plays_a_default_architecture_file_at_a_temperature(tmp_path, capsys):
    """the real command line on a file of the default architecture (1 fc layer, 2 LSTM layers: what clone and selfplay write, and what
    the loader seats as the bf16 r2d2.R2D2Agent) in the standard game, self-play and the matrix with a bot: the recorded games hold
    moves that are not the greedy ones, --temperature 0 none, and the bot's entry is ignored"""
    from hanabi_sad_amd import eval_model, game_record as gr
    from hanabi_sad_amd.eval import env_dims
    from hanabi_sad_amd.r2d2 import R2D2Agent
    from hanabi_sad_amd.selfplay import init_weights
    F, A = env_dims(2, 5, True)
    files = []
    for k in range(2):
        files.append(str(tmp_path / ("w%d.pthw" % k)))
        torch.save(init_weights(F, 64, A, 5, 40 + k), files[-1])
    args = eval_model.parse_args(["--paper", "sad", "--weight", files[0], "--device", DEV])
    assert type(eval_model.load_pool(args)[0][0]) is R2D2Agent
    left = {}
    for t in ("1", "0"):
        games = str(tmp_path / ("games%s.jsonl" % t))
        res = eval_model.main(["--paper", "sad", "--weight", files[0], "--num_game", "32", "--temperature", t, "--sample_seed", "9", "--device", DEV,
                               "--save_games", games])
        assert re.search(r"score: [0-9.]+ \+/- [0-9.]+", capsys.readouterr().out) and res.scores.shape == (1, 32)
        records = gr.load(games)
        assert len(records) == 32
        left[t] = sum(a != g for r in records for a, g in zip(r.moves, r.greedy))
    print("self-play moves that are not the greedy one: temperature 1: %d, temperature 0: %d" % (left["1"], left["0"]))
    assert left["1"] > 0 and left["0"] == 0
    games = str(tmp_path / "matrix.jsonl")
    res = eval_model.main(["--paper", "sad", "--weight", files[0], files[1], "--cross_play", "--bots", "piers", "--num_game", "16", "--temperature", "0", "1",
                           "--device", DEV, "--save_games", games])
    assert "self-play & cross-play" in capsys.readouterr().out and res.mean.shape == (3, 3)
    by_seat = {0: 0, 1: 0}
    for r in gr.load(games):
        for i, (a, g) in enumerate(zip(r.moves, r.greedy)):
            by_seat[r.meta["seats"][i % 2] == "W1"] += a != g
    assert by_seat[1] > 0 and by_seat[0] == 0, by_seat
    for argv, text in ((["--temperature", "0.5", "1", "0"], "one value or one per model"), (["--temperature", "-1"], "not negative")):
        with pytest.raises(SystemExit, match=text):
            eval_model.main(["--paper", "sad", "--weight", files[0], files[1], "--cross_play", "--num_game", "4", "--device", DEV] + argv)
