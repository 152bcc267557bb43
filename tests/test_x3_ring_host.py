"""K11x's index carry on the CPU: the stand-alone program over
csrc/kernels/x3_ring_math.h, and tools/isa_loop_stats.py on a small listing."""
import os
import subprocess
import sys
import textwrap

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_stand_alone_cpp_test_passes():
    """csrc/cpp/tests/x3_ring_test.cc, as the project's build makes it (the
    ``asan`` preset builds the same source with the sanitizers)."""
    exe = os.path.join(REPO, "csrc", "cpp", "build", "bin", "x3_ring_test")
    assert os.path.exists(exe), "csrc/cpp is not built"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith(" 0 failures"), r.stdout[-2000:] + r.stderr[-2000:]


LISTING = """\
    .text
    .globl  toy
toy:
    s_load_dwordx2 s[0:1], s[4:5], 0x0
    v_mov_b32_e32 v0, 0
    s_waitcnt lgkmcnt(0)
.LBB0_1:
    ds_read_b128 v[4:7], v1 offset:544
    v_mul_lo_u32 v2, v2, s0
    v_cndmask_b32_e32 v3, v3, v2, vcc
    s_waitcnt lgkmcnt(0)
    v_mfma_f32_16x16x32_bf16 v[8:11], v[4:7], v[4:7], v[8:11]
    s_add_i32 s2, s2, 1
    s_cmp_lt_i32 s2, s3
    s_cbranch_scc1 .LBB0_1
    global_store_dword v0, v8, s[0:1]
    s_endpgm
    .amdhsa_kernel toy
    .end_amdhsa_kernel
.Lfunc_end0:
    ; -- End function
    .amdgpu_metadata
---
amdhsa.kernels:
  - .name:           toy
    .vgpr_count:     12
    .vgpr_spill_count: 0
    .private_segment_fixed_size: 0
    .end_amdgpu_metadata
"""


def test_isa_loop_stats_counts_a_loop(tmp_path):
    import json

    f = tmp_path / "toy.s"
    f.write_text(textwrap.dedent(LISTING).replace("    .end_amdgpu_metadata", "\t.end_amdgpu_metadata"))
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "isa_loop_stats.py"), str(f), "toy", "--json",
                        "--min", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout)
    assert got["meta"]["vgpr_count"] == 12 and got["meta"]["vgpr_spill_count"] == 0
    loop = [x for x in got["regions"] if x["loop"]]
    assert len(loop) == 1 and loop[0]["depth"] == 1
    assert {k: loop[0][k] for k in ("mfma", "valu", "mul", "cnd", "lds", "salu", "wait", "vmem")} == {
        "mfma": 1, "valu": 2, "mul": 1, "cnd": 1, "lds": 1, "salu": 3, "wait": 1, "vmem": 0}
    assert got["total"]["vmem"] == 1 and got["total"]["mfma"] == 1
