"""Static checks on the compiled gfx950 code of the wave priority in the pipelined persistent rollout (env_rollout_pipe_kernel,
hsad_env_set_rollout_prio; no GPU needed: hipcc cross-compiles).  s_setprio takes an immediate and ignores EXEC, so the kernel
reaches one of four of them through scalar branches at the top of every iteration: each pipelined instance must hold all four inside
its iteration loop, at the register counts the instances had before (two waves per SIMD, four workgroups per CU) and without
scratch; the kernels the change does not touch hold none."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# vgpr_count of the pipelined instances on the parent commit (tools/isa_compare.py)
PARENT_VGPRS = {"env_rollout_pipe_kernelILi2ELi5E": 176, "env_rollout_pipe_kernelILi5ELi4E": 204, "env_rollout_pipe_kernelILi3ELi5E": 176,
                "env_rollout_pipe_kernelILi4ELi4E": 197, "env_rollout_pipe_kernelILi0ELi0E": 233}
UNTOUCHED = ("env_rollout_kernelILi2ELi5ELb0E", "env_kernelILi3ELi2ELi5ELb0E")


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
    m = re.search(r"^(\S*\d%s\S*):[^\n]*\n(.*?)\n\s*s_endpgm" % needle, text, re.S | re.M)
    assert m, needle + " body not found"
    return m.group(2).split("\n")


def loop_header_of(lines, i):
    """the header of the innermost loop the basic block of line i belongs to, as the compiler annotates the block; None outside loops"""
    while i >= 0:
        if lines[i].startswith(".LBB") or lines[i].startswith("; %bb."):
            note = lines[i]                      # the label's comment and the comment-only lines that continue it
            j = i + 1
            while j < len(lines) and lines[j].lstrip().startswith(";") and not lines[j].startswith("; %bb."):
                note += lines[j]
                j += 1
            m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", note)
            if m:
                return m.group(1), int(m.group(2))
            m = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", note)   # the block is a loop's own header
            if m:
                return lines[i].split(":")[0].replace(".L", ""), int(m.group(1))
            return None
        i -= 1
    return None


@pytest.mark.parametrize("kernel", sorted(PARENT_VGPRS))
def test_four_setprio_forms_inside_the_iteration_loop(env_isa, kernel):
    lines = body(env_isa, kernel)
    prio = [(i, l.split()[1]) for i, l in enumerate(lines) if l.strip().startswith("s_setprio")]
    assert sorted(p for _, p in prio) == ["0", "1", "2", "3"], prio
    headers = {loop_header_of(lines, i) for i, _ in prio}
    assert len(headers) == 1 and None not in headers, headers           # one loop holds all four ...
    header, depth = headers.pop()
    assert depth == 1, (header, depth)                                    # ... the outermost one: the launch's iterations
    # and it is the loop the two barriers of an iteration are in
    bars = [i for i, l in enumerate(lines) if l.strip() == "s_barrier"]
    in_loop = [i for i in bars if (loop_header_of(lines, i) or (None, 0))[0] == header]
    assert len(in_loop) >= 2, (header, len(bars), len(in_loop))
    # every s_setprio stands behind a scalar branch, not under an exec mask alone
    branches = [l for l in lines[prio[0][0] - 40:prio[-1][0]] if re.match(r"\s*s_cbranch_(scc|vcc)", l)]
    assert len(branches) >= 3, branches


@pytest.mark.parametrize("kernel", sorted(PARENT_VGPRS))
def test_registers_are_the_parents_and_no_scratch(env_isa, kernel):
    md = meta(env_isa, kernel)
    assert md["vgpr_count"] == PARENT_VGPRS[kernel], md
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0, md


@pytest.mark.parametrize("kernel", UNTOUCHED)
def test_other_kernels_hold_no_setprio(env_isa, kernel):
    lines = body(env_isa, kernel)
    assert len(lines) > 1000, kernel
    assert not [l for l in lines if "s_setprio" in l], kernel
