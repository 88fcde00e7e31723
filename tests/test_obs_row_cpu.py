"""csrc/hsad_obs_row.h without a device: an observer's row assembled at fixed bit positions and placed with one shifted write,
compiled alone under the address and undefined-behaviour sanitizers and held word for word to the scatter form of build_rows
(tests/obs_row/obs_row_main.cc restates it), for every fixed (players, hand) instance, SAD on and off, identity and shuffled
colours.  The kernel that uses the header is held to the scatter kernels on the device in test_env_rollout_rowbuild_gpu.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("obs_row") / "obs_row_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "hanabi_sad_amd", "csrc"),
                           os.path.join(ROOT, "tests", "obs_row", "obs_row_main.cc"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    words = out.stdout.split()
    return {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}


def test_rows_agree_with_the_scatter_form(counts):
    # 4 instances x sad 0 / 1 x identity / shuffled x (1000+ random states and 40 extremes), every observer in three placements
    assert counts["rows"] >= 16 * 1000 * 2 * 3
    assert counts["extremes"] == 16 * 40


def test_every_shift_and_the_buffer_ends(counts):
    # all 32 values of base & 31; rows placed first in the buffer, and last, ending on its last word with guard words behind
    assert counts["shifts"] == 32
    assert counts["first"] >= 16 * 1000 * 2 and counts["last"] >= 16 * 1000 * 2
