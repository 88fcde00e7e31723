"""GPU: python -m hanabi_sad_amd.belief end to end on 32 games of the `piers` bot for 2 epochs with a 64-unit blueprint: every epoch
line carries the NLL per card and the top-1 accuracy of the learned and of the exact belief on both sides of the split, the first
epoch starts from the exact belief, and the file it writes loads into a head of the same shape."""
import os
import re

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
DEV = "cuda:0"
LINE = re.compile(r"epoch (\d+): NLL per card ([0-9.]+) \(exact belief ([0-9.]+)\), top-1 ([0-9.]+) \(exact ([0-9.]+)\); held out: NLL per card "
                  r"([0-9.]+) \(exact belief ([0-9.]+)\), top-1 ([0-9.]+) \(exact ([0-9.]+)\)")


def test_the_driver_trains_prints_both_columns_and_writes_a_loadable_head(tmp_path, capsys):
    from hanabi_sad_amd import belief
    from hanabi_sad_amd.checkpoint import save_weights
    from hanabi_sad_amd.eval import env_dims
    from hanabi_sad_amd.selfplay import init_weights
    F, A = env_dims(2, 5, True)
    W = init_weights(F, 64, A, 5, 9)
    blueprint = str(tmp_path / "blueprint.pthw")
    save_weights(W, blueprint)
    out_dir = str(tmp_path / "run")
    rc = belief.main(["--blueprint", blueprint, "--teacher", "piers", "--num_game", "32", "--sad", "1", "--num_epoch", "2", "--batchsize", "16",
                      "--holdout", "0.25", "--lr", "0.01", "--save_dir", out_dir, "--train_device", DEV])
    assert rc == 0
    text = capsys.readouterr().out
    print(text)
    assert "32 games" in text and "held out" in text
    lines = [LINE.search(l) for l in text.splitlines() if l.startswith("epoch")]
    assert len(lines) == 2 and all(lines)
    vals = [[float(x) for x in m.groups()[1:]] for m in lines]
    for nll, nll0, top1, top1_0, h_nll, h_nll0, h_top1, h_top1_0 in vals:
        assert 0 < nll0 < 10 and 0 < h_nll0 < 10 and 0 <= top1_0 <= 1 and 0 <= h_top1_0 <= 1 and nll > 0 and h_nll > 0
    assert vals[0][1] == vals[1][1] and vals[0][5] == vals[1][5]      # the exact belief's columns do not move
    assert os.path.isfile(os.path.join(out_dir, "games.jsonl"))
    sd = torch.load(os.path.join(out_dir, "belief.pthw"), map_location="cpu")
    assert belief.check_state(sd) == (5, 64) and float(sd["belief.weight"].abs().sum()) > 0
    head = belief.BeliefHead(blueprint, 5, DEV).load(os.path.join(out_dir, "belief.pthw"))
    assert torch.equal(head.weight.cpu(), sd["belief.weight"])
    # --games takes the file the run left
    rc = belief.main(["--blueprint", blueprint, "--games", os.path.join(out_dir, "games.jsonl"), "--seat", "0", "--num_epoch", "1", "--batchsize", "16",
                      "--holdout", "0.25", "--train_device", DEV])
    assert rc == 0 and "32 sequences" in capsys.readouterr().out
