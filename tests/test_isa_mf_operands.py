"""Static check of the operand stream of the 4-tile wave kernel (mf_mfma_wave_kernel, NTILE == 4) in the generated gfx950
ISA: the K loop is one basic block of 16 MFMAs fed by 8 ds_read_b64 (B: the four-phase window, two k-steps per read) and 2
ds_read2_b32 (A), nothing of the kernel lives in scratch, the accumulators are zeroed once per channel, and no instruction
touches a register that a hand-issued read still has in flight (tools/check_inflight.py).  Runs on CPU: hipcc cross-compiles
mf.hip to an assembly listing."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_inflight  # noqa: E402

HEADLINE = "mf_mfma_wave_kernelILb1ELi20ELi5ELb1ELi4ELb0ELb0E"


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from seismic_bpmf_amd.build import ARCH, CSRC, find_hipcc
    out = tmp_path_factory.mktemp("isa") / "mf.s"
    cmd = [find_hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-ffp-contract=off", "-S",
           "--cuda-device-only", "-o", str(out), os.path.join(CSRC, "mf.hip")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    return out.read_text()


def _four_tile_kernels(text):
    """{name: instructions} of the wave kernel's instantiations with 4 tiles per wave: <NS, 20, 5, S1, 4, ...>"""
    kernels = check_inflight.split_kernels(text)
    return {n: b for n, b in kernels.items() if re.search(r"mf_mfma_wave_kernelILb[01]ELi20ELi5ELb[01]ELi4E", n)}


def _blocks(body):
    """Basic blocks of a kernel in listing order, without the inline-asm markers."""
    blocks, _ = check_inflight._blocks(body)
    return [[t for t in b if not t.startswith("#ASM")] for _, b in blocks]


@pytest.mark.timeout(900)
def test_k_loop_reads_operands_by_pairs_of_k_steps(listing):
    kernels = _four_tile_kernels(listing)
    assert len(kernels) >= 8, sorted(kernels)             # network sum x step 1 x normalisation, at least
    assert sum(HEADLINE in n for n in kernels) == 1
    for n, body in kernels.items():
        assert not any("scratch_" in t for t in body), n
        blocks = _blocks(body)
        loops = [i for i, b in enumerate(blocks) if any(t.startswith("v_mfma") for t in b)]
        assert len(loops) == 1, n                         # every MFMA of the kernel is in one block ...
        loop = blocks[loops[0]]
        count = lambda op: sum(t.split()[0] == op for t in loop)  # noqa: E731
        assert count("v_mfma_f32_16x16x4_f32") == 16, n
        assert re.match(r"s_cbranch_\w+", loop[-1].split()[0]), (n, loop[-1])     # ... which is a loop: it ends in its back edge
        assert count("ds_read_b64") == 8 and count("ds_read2_b32") == 2 and count("ds_read_b32") == 0, n
        assert not any(re.match(r"s_waitcnt\s.*lgkmcnt\(0\)", t) for t in loop), n
        # the accumulators are zeroed once per channel: in the block that falls into the loop, at most 16 moves of a zero
        # (of the constant, or of a register that block has just set to it)
        zero_regs, zero_moves = set(), 0
        for t in blocks[loops[0] - 1]:
            m = re.match(r"v_mov_b32_e32\s+(v\d+),\s*(\S+)$", t)
            if m and (m.group(2) == "0" or m.group(2) in zero_regs):
                zero_regs.add(m.group(1))
                zero_moves += 1
        assert zero_moves <= 16, (n, zero_moves)
        bad = check_inflight.check_kernel(body)
        assert not bad, f"{n}: {bad[:4]}"


@pytest.mark.timeout(900)
def test_headline_kernel_keeps_its_registers(listing):
    meta = listing[listing.index("amdhsa.kernels"):]
    head = [b for b in meta.split("  - .agpr_count")[1:] if HEADLINE in b]
    assert len(head) == 1
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", head[0]).group(1)) <= 125
    assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", head[0]).group(1)) == 0
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", head[0]).group(1)) == 0
