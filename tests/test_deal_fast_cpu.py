"""csrc/hsad_deal_fast.h without a device: the deal's pick on the packed deck, the policy's k-th legal bit and the wrapped mt19937
window index, compiled alone under the address and undefined-behaviour sanitizers and held to the scans they replace
(tests/deal_fast/deal_fast_main.cc restates them).  The kernels that use the header are held to the oracle and to the literal deal
path in test_env_parity_gpu.py and test_env_rollout_logic_gpu.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("deal_fast") / "deal_fast_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "hanabi_sad_amd", "csrc"),
                           os.path.join(ROOT, "tests", "deal_fast", "deal_fast_main.cc"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    words = out.stdout.split()
    return {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}


def test_pick_agrees_with_the_scan_on_every_need_of_every_deck(counts):
    # 49 sizes x 230 random decks and the hand-written ones; every need 1..D of each
    assert counts["decks"] >= 10000 + 100
    assert counts["picks"] >= 26 * 10000


def test_select_agrees_with_the_loop_on_every_k(counts):
    assert counts["masks"] >= 16000 + 4 * 4000
    assert counts["selects"] > 20 * counts["masks"] // 2


def test_wrapped_index_is_the_remainder(counts):
    assert counts["wraps"] == 624 * (64 + 397 + 1)
