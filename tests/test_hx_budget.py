"""Register budget of the conv_hx instances that run two workgroups per CU (csrc/fastsvc_hx.hip, hx_min_waves / hx_two_cu).

An 8-wave workgroup fits a CU twice only at <= 128 VGPRs per lane.  hipcc keeps the bound it is given
(__launch_bounds__(512, 4)) by spilling, so the thing to hold is "within the bound WITHOUT a spill or scratch": a later
change that pushes one of these instances over the line fails here instead of showing up as a silent 20 % on the GPU.
No GPU needed: the objects are those of the build (hipcc cross-compiles)."""
import glob
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from svcc23_fastsvc_amd import build as B          # noqa: E402
import kernel_resources                            # noqa: E402

# (MW, NW, WM, WN, MODE, EPI, S, WSTATIC, TAILK) as conv_hx_kernel's template arguments; MODE 0 = direct, EPI 4 = FiLM
# affine, 1 / 2 / 3 = plain / residual tensor / rank-1 residual; S > 1 = the second (stretched) operand of a d3x launch
TWO_PER_CU = [
    # the C = 48 FiLM-affine convs (hx_two_cu): up.2.d9 | d3x with a x2 and a x4 second operand
    "conv_hx_kernel<3, 2, 1, 4, 0, 4, 1, false, false>",
    "conv_hx_kernel<3, 2, 1, 4, 0, 4, 2, false, false>",
    "conv_hx_kernel<3, 2, 1, 4, 0, 4, 4, false, false>",
    # the C = 24 convs: FiLM affine with the x5 second operand (up.3.d3x), plain / residual / rank-1 (one and more K chunks)
    "conv_hx_kernel<2, 2, 1, 4, 0, 4, 5, true, false>",
    "conv_hx_kernel<2, 2, 1, 4, 0, 1, 1, true, false>",
    "conv_hx_kernel<2, 2, 1, 4, 0, 2, 1, true, false>",
    "conv_hx_kernel<2, 2, 1, 4, 0, 3, 1, true, false>",
    "conv_hx_kernel<2, 2, 1, 4, 0, 1, 1, false, false>",
    "conv_hx_kernel<2, 2, 1, 4, 0, 2, 1, false, false>",
    "conv_hx_kernel<2, 2, 1, 4, 0, 3, 1, false, false>",
]
# instances that stay at one workgroup per CU on purpose: the float32 twins and the row-end (TAILK) twin keep their budget
ONE_PER_CU_F32 = ["conv_hx_kernel<3, 2, 1, 4, 0, 4, 1, false, false>", "conv_hx_kernel<3, 2, 1, 4, 0, 4, 4, false, false>"]


def _object(stem):
    """the build cache's object of a unit (svcc23_fastsvc_amd/build/<stem>_<key>.o), compiled here if the cache lacks it"""
    B.build()                                                      # (no-op when the library is up to date)
    cache = os.path.join(B.PKG_DIR, "build")
    hits = [p for p in glob.glob(os.path.join(cache, stem + "_*.o")) if len(os.path.basename(p)) == len(stem) + 19]
    if hits:
        return max(hits, key=os.path.getmtime)
    src, extra, _ = next(u for u in B.UNITS if u[2] == stem + ".o")
    os.makedirs(cache, exist_ok=True)
    out = os.path.join(cache, stem + "_budgettest.o")
    subprocess.run([B._hipcc(), f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics",
                    "-I", os.path.join(B.ROOT, "include"), "-I", B.CSRC, *extra, "-x", "hip", "-c",
                    os.path.join(B.CSRC, src), "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def tables():
    return {stem: kernel_resources.table(_object(stem)) for stem in ("hx_bf16", "hx_f16", "hx_f32")}


@pytest.mark.parametrize("stem,ns", [("hx_bf16", "bf16::"), ("hx_f16", "f16::")])
@pytest.mark.parametrize("inst", TWO_PER_CU)
def test_two_per_cu_instances_fit_128_registers_without_spilling(tables, stem, ns, inst):
    r = tables[stem][ns + inst]
    print(f"{stem} {inst}: {r}")
    assert r["vgpr"] <= 128, r
    assert r["vspill"] == 0 and r["scratch"] == 0, r


def test_two_workgroups_fit_the_lds_of_a_cu():
    """hx_launch_shape's dynamic LDS of the C = 48 FiLM-affine instances (2-byte storage, no residual operand) plus the
    static part, for every dilation the kernel takes: at most half of a CU's 160 KB."""
    MW, NW, WN, KC32 = 3, 2, 4, 2
    for dil in range(1, 28):
        halo_al = (dil + 7) & ~7
        W = 16 * NW * WN + 2 * halo_al
        smem = 8 * 2 * 16 * MW + 4 * 2 * (KC32 * 32 + 8) + 2 * (W + 8) * 64        # sums | prologue coefficients | two windows
        smem += 4 * 4 * 2 * (MW * (NW // 2) * 256)                                # scale and shift slots of four waves
        smem += 4 * 4 * 16 * 36                                                    # re-layout patches
        smem += 4 * MW * 2 * 64 * 8                                                # the lanes' float64 InstanceNorm sums
        assert smem + 4096 <= 80 * 1024, (dil, smem)


def test_float32_twins_keep_their_budget(tables):
    for inst in ONE_PER_CU_F32:
        r = tables["hx_f32"][inst]
        assert r["vgpr"] > 128 and r["vspill"] == 0 and r["scratch"] == 0, (inst, r)
