"""Static checks on the compiled gfx950 code of the pipelined persistent rollout (env_rollout_pipe_kernel; no GPU needed: hipcc
cross-compiles).  The schedule only pays if all 1,024 workgroups of configs[1] stay resident, four per CU: no scratch and two waves
per SIMD (at most 256 VGPRs under amdgpu_waves_per_eu(2, 2)); the LDS fit of four workgroups is checked on the library's own sizing in
test_env_rollout_pipeline_gpu.py.  Its barriers must stay LDS-only: a vmcnt(0) in front of one would make the stream wave wait for its own stores, i.e. serialise the two phases again."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("env_rollout_pipe_kernelILi2ELi5E", "env_rollout_pipe_kernelILi5ELi4E", "env_rollout_pipe_kernelILi3ELi5E",
           "env_rollout_pipe_kernelILi4ELi4E", "env_rollout_pipe_kernelILi0ELi0E")


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


def body(text, needle):
    m = re.search(r"^(\S*%s\S*):[^\n]*\n(.*?)\n\s*s_endpgm" % needle, text, re.S | re.M)
    assert m, needle + " body not found"
    return m.group(2).split("\n")


@pytest.mark.parametrize("kernel", KERNELS)
def test_pipelined_rollout_has_no_scratch_and_two_waves_per_simd(env_isa, kernel):
    md = meta(env_isa, kernel)
    # (SGPR spills land in VGPR lanes, as in env_rollout_kernel; only a VGPR spill or a private segment means scratch)
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, md
    assert md["vgpr_count"] <= 256, md                       # 512 VGPRs per SIMD lane / 256 = 2 waves per SIMD


def test_configs1_pipelined_rollout_uses_no_more_registers_than_the_single_phase_one(env_isa):
    assert meta(env_isa, "env_rollout_pipe_kernelILi2ELi5E")["vgpr_count"] <= meta(env_isa, "env_rollout_kernelILi2ELi5E")["vgpr_count"]


def test_pipelined_rollout_barriers_wait_for_lds_only(env_isa):
    for kernel in ("env_rollout_pipe_kernelILi2ELi5E", "env_rollout_pipe_kernelILi5ELi4E"):
        lines = body(env_isa, kernel)
        bars = [i for i, l in enumerate(lines) if l.strip() == "s_barrier"]
        assert len(bars) >= 3, kernel                         # prologue, end of phase A, end of phase B
        for i in bars:
            # every instruction from the start of the barrier's basic block (label or the previous barrier) up to the barrier
            j = i - 1
            while j >= 0 and not lines[j].startswith(".LBB") and lines[j].strip() != "s_barrier":
                assert not (lines[j].strip().startswith("s_waitcnt") and "vmcnt" in lines[j]), \
                    "%s: %s in the block of a barrier" % (kernel, lines[j].strip())
                j -= 1
