"""Register / LDS / scratch budget of the attention kernels (hipcc -Rpass-analysis=kernel-resource-usage, no GPU needed;
the mechanism of tests/test_kernel_resources.py).

graphtrans_amd/csrc/attention.hip carries one exact instantiation of k_attn_fwd / k_attn_bwd_dq / k_attn_bwd_dkv per head
dim (every multiple of 8 up to 128), storage type and mask form.  What is pinned here:
  * the instantiations that serve head dim 128 exist, for both storage types;
  * nothing in the file spills to scratch, and the bf16 kernels at head dim 128 keep two blocks per CU;
  * the 54 instantiations that existed before the head-dim set was widened (8 / 16 / 32 / 64) are still there with the
    occupancy and the LDS size they had (PARENT below: VGPRs, waves per SIMD, LDS bytes per block, measured with the same
    hipcc before the change; the VGPR counts are printed beside today's, occupancy and LDS are asserted)."""
import functools
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graphtrans_amd", "csrc")

# (kernel, storage type 'f' = float / 't' = bf16, head dim, dense masks, bf16x6 products): (VGPRs, waves per SIMD, LDS bytes)
PARENT = {
    ('bwd_dkv', 'f', 8, 0, 0): (110, 4, 19200), ('bwd_dkv', 'f', 8, 1, 0): (116, 4, 19200),
    ('bwd_dkv', 'f', 16, 0, 0): (114, 4, 19200), ('bwd_dkv', 'f', 16, 1, 0): (120, 4, 19200),
    ('bwd_dkv', 'f', 32, 0, 0): (134, 3, 19200), ('bwd_dkv', 'f', 32, 0, 1): (148, 3, 31488),
    ('bwd_dkv', 'f', 32, 1, 0): (138, 3, 19200), ('bwd_dkv', 'f', 64, 0, 0): (167, 3, 35584),
    ('bwd_dkv', 'f', 64, 0, 1): (232, 2, 56064), ('bwd_dkv', 'f', 64, 1, 0): (173, 2, 35584),
    ('bwd_dkv', 't', 8, 0, 0): (84, 5, 11008), ('bwd_dkv', 't', 8, 1, 0): (92, 5, 11008),
    ('bwd_dkv', 't', 16, 0, 0): (86, 5, 11008), ('bwd_dkv', 't', 16, 1, 0): (94, 5, 11008),
    ('bwd_dkv', 't', 32, 0, 0): (94, 5, 11008), ('bwd_dkv', 't', 32, 1, 0): (102, 4, 11008),
    ('bwd_dkv', 't', 64, 0, 0): (124, 4, 19200), ('bwd_dkv', 't', 64, 1, 0): (132, 3, 19200),
    ('bwd_dq', 'f', 8, 0, 0): (88, 5, 18432), ('bwd_dq', 'f', 8, 1, 0): (94, 5, 18432),
    ('bwd_dq', 'f', 16, 0, 0): (94, 5, 18432), ('bwd_dq', 'f', 16, 1, 0): (98, 4, 18432),
    ('bwd_dq', 'f', 32, 0, 0): (98, 4, 18432), ('bwd_dq', 'f', 32, 0, 1): (110, 4, 30720),
    ('bwd_dq', 'f', 32, 1, 0): (102, 4, 18432), ('bwd_dq', 'f', 64, 0, 0): (126, 4, 34816),
    ('bwd_dq', 'f', 64, 0, 1): (166, 2, 55296), ('bwd_dq', 'f', 64, 1, 0): (128, 4, 34816),
    ('bwd_dq', 't', 8, 0, 0): (61, 8, 10240), ('bwd_dq', 't', 8, 1, 0): (70, 7, 10240),
    ('bwd_dq', 't', 16, 0, 0): (66, 7, 10240), ('bwd_dq', 't', 16, 1, 0): (72, 7, 10240),
    ('bwd_dq', 't', 32, 0, 0): (70, 7, 10240), ('bwd_dq', 't', 32, 1, 0): (78, 6, 10240),
    ('bwd_dq', 't', 64, 0, 0): (92, 5, 18432), ('bwd_dq', 't', 64, 1, 0): (98, 4, 18432),
    ('fwd', 'f', 8, 0, 0): (77, 6, 18432), ('fwd', 'f', 8, 1, 0): (81, 5, 18432),
    ('fwd', 'f', 16, 0, 0): (84, 5, 18432), ('fwd', 'f', 16, 1, 0): (87, 5, 18432),
    ('fwd', 'f', 32, 0, 0): (104, 4, 18432), ('fwd', 'f', 32, 0, 1): (112, 4, 30720),
    ('fwd', 'f', 32, 1, 0): (106, 4, 18432), ('fwd', 'f', 64, 0, 0): (118, 4, 34816),
    ('fwd', 'f', 64, 0, 1): (154, 2, 55296), ('fwd', 'f', 64, 1, 0): (121, 4, 34816),
    ('fwd', 't', 8, 0, 0): (62, 8, 10240), ('fwd', 't', 8, 1, 0): (64, 8, 10240),
    ('fwd', 't', 16, 0, 0): (68, 7, 10240), ('fwd', 't', 16, 1, 0): (70, 7, 10240),
    ('fwd', 't', 32, 0, 0): (78, 6, 10240), ('fwd', 't', 32, 1, 0): (80, 6, 10240),
    ('fwd', 't', 64, 0, 0): (92, 5, 18432), ('fwd', 't', 64, 1, 0): (94, 5, 18432),
}
KERNELS = ("fwd", "bwd_dq", "bwd_dkv")


@functools.lru_cache(maxsize=None)
def _usage():
    """{(kernel, storage type, head dim, dense, bf16x6): {VGPRs, AGPRs, ScratchSize, Occupancy, LDS}} of attention.hip"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", os.path.join(CSRC, "attention.hip"), "-o", os.devnull,
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=CSRC).stderr
    kernels, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = None
            k = re.search(r"\d+k_attn_(fwd|bwd_dq|bwd_dkv)I([ft])Li(\d+)ELb([01])ELb([01])E", m.group(1))
            if k:
                cur = kernels.setdefault((k.group(1), k.group(2), int(k.group(3)), int(k.group(4)), int(k.group(5))), {})
            else:
                assert "k_attn_" not in m.group(1), "attention kernel with a signature this test does not know: " + m.group(1)
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    assert kernels, out[-2000:]
    return kernels


def test_head_dim_128_has_instantiations_of_all_three_kernels():
    k = _usage()
    for kern in KERNELS:
        for t in "ft":
            for dense in (0, 1):
                assert (kern, t, 128, dense, 0) in k, f"no k_attn_{kern} for head dim 128, storage {t}, dense masks {dense}"
    # every head dim of the accepted set is an exact instantiation
    for hd in range(8, 129, 8):
        for kern in KERNELS:
            for t in "ft":
                assert (kern, t, hd, 0, 0) in k and (kern, t, hd, 1, 0) in k, (kern, t, hd)


def test_no_attention_kernel_spills_and_bf16_at_128_keeps_two_blocks_per_cu():
    k = _usage()
    spills = {n: v["ScratchSize"] for n, v in k.items() if v.get("ScratchSize", 0) > 0}
    assert not spills, "attention kernels spilling to scratch: %s" % spills
    for kern in KERNELS:
        for dense in (0, 1):
            v = k[(kern, "t", 128, dense, 0)]
            print(f"k_attn_{kern}<bf16, 128, dense={dense}>: {v['VGPRs']} VGPRs + {v.get('AGPRs', 0)} AGPRs, {v['Occupancy']} waves per SIMD, "
                  f"{v['LDS']} B of LDS")
            assert v["Occupancy"] >= 2, (kern, dense, v)
            assert v["VGPRs"] + v.get("AGPRs", 0) <= 256, (kern, dense, v)
            assert 2 * v["LDS"] <= 160 * 1024, (kern, dense, v)   # two blocks per CU by LDS as well


def test_the_earlier_instantiations_keep_their_occupancy_and_lds():
    k = _usage()
    assert len(PARENT) == 54
    bad = []
    for key, (vgprs, occ, lds) in sorted(PARENT.items()):
        assert key in k, f"instantiation {key} is gone"
        v = k[key]
        mark = "" if v["VGPRs"] == vgprs else "   <- VGPRs changed"
        print(f"{key}: VGPRs {v['VGPRs']} (was {vgprs}), waves per SIMD {v['Occupancy']} (was {occ}), LDS {v['LDS']} (was {lds}){mark}")
        if v["Occupancy"] != occ or v["LDS"] != lds or v.get("AGPRs", 0) != 0:
            bad.append((key, v))
    assert not bad, bad
