"""Static checks on the logic wave's code in the pipelined persistent rollout (env_rollout_pipe_kernel; no GPU needed: hipcc
cross-compiles).  The logic wave is bound by the number of instructions it executes on paths the whole wave walks every iteration
(DESIGN 3a), so the flagship instance's code must not grow back past what it was before its reset, deal and policy paths were
cut: 71,712 bytes.  The carried policy keys and the straight deal must not push any pipelined instance into scratch either."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("env_rollout_pipe_kernelILi2ELi5E", "env_rollout_pipe_kernelILi5ELi4E", "env_rollout_pipe_kernelILi3ELi5E",
           "env_rollout_pipe_kernelILi4ELi4E", "env_rollout_pipe_kernelILi0ELi0E")
CODE_BYTES_BEFORE = 71712     # env_rollout_pipe_kernel<2,5> with the 65 `% 624` addresses, the generator-call deal and three mix64 per pick


@pytest.fixture(scope="module")
def env_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = str(tmp_path_factory.mktemp("isa") / "hsad_env.s")
    src = os.path.join(ROOT, "hanabi_sad_amd", "csrc", "hsad_env.hip")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-inline-asm",
                           "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S", "-o", out, src],
                          stderr=subprocess.DEVNULL)
    return open(out).read()


def meta(text, needle):
    m = re.search(r"\.name:\s+(\S*%s\S*)\n(.*?)\.wavefront_size" % needle, text, re.S)
    assert m, needle + " not found in the assembly"
    return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\n", m.group(2))}


def code_bytes(text, needle):
    m = re.search(r"^(\S*%s\S*):.*?\n\.Lfunc_end\d+:.*?codeLenInByte = (\d+)" % needle, text, re.S | re.M)
    assert m, needle + " body not found"
    return int(m.group(2))


def test_flagship_instance_is_no_longer_than_before(env_isa):
    n = code_bytes(env_isa, "env_rollout_pipe_kernelILi2ELi5E")
    print("env_rollout_pipe_kernel<2,5>: %d bytes of code" % n)
    assert n <= CODE_BYTES_BEFORE


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_pipelined_instance_spills_vector_registers(env_isa, kernel):
    md = meta(env_isa, kernel)
    assert md["vgpr_spill_count"] == 0 and md["private_segment_fixed_size"] == 0, md
