"""Register / scratch budget of the PNA baseline's head kernels (csrc/mlp_heads.hip), the pattern of tests/test_kernel_resources.py:
hipcc -Rpass-analysis=kernel-resource-usage, no GPU needed.  The grouped forward and dH kernels hold 16 accumulator tiles and eight
operand fragments per wave in 512-thread blocks (256 registers per lane at the most); nothing may spill to scratch."""
import re

from test_kernel_resources import _usage


def test_head_kernels_do_not_spill():
    k = _usage("mlp_heads.hip")
    names = " ".join(k)
    for kernel in ("k_hg_fwd", "k_hg_dx", "k_hg_dx_reduce", "k_hg_dw", "k_mlp_fwd", "k_mlp_bwd_rows", "k_mlp_bwd_params"):
        assert kernel in names, (kernel, sorted(k))
    assert len([n for n in k if re.search(r"k_hg_(fwd|dx|dw)I[ft]E", n)]) == 6   # fp32 and bf16 operands of the three MFMA kernels
    spills = {n: v["ScratchSize"] for n, v in k.items() if v.get("ScratchSize", 0) > 0}
    assert not spills, "head kernels spilling to scratch: %s" % spills
    for n, v in k.items():
        if re.search(r"k_hg_(fwd|dx)I", n):   # 8 waves per block: two per SIMD
            assert v["VGPRs"] + v.get("AGPRs", 0) <= 256 and v["Occupancy"] >= 2, (n, v)
