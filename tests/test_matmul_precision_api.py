"""ops.set_matmul_precision / get_matmul_precision, the GT_F32_PRECISION default and the gt_compute value behind "high" (no GPU)."""
import os
import re
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_set_get_round_trip_and_bad_values():
    from graphtrans_amd import ops
    start = ops.get_matmul_precision()
    try:
        assert ops.set_matmul_precision("high") == start
        assert ops.get_matmul_precision() == "high"
        assert ops.set_matmul_precision("highest") == "high"
        assert ops.get_matmul_precision() == "highest"
        for bad in ("medium", "HIGH", None, 2):
            with pytest.raises(ValueError):
                ops.set_matmul_precision(bad)
        assert ops.get_matmul_precision() == "highest"   # a rejected value changes nothing
    finally:
        ops.set_matmul_precision(start)


def test_compute_code_follows_dtype_then_precision():
    from graphtrans_amd import _lib, layers, ops
    start = ops.get_matmul_precision()
    try:
        ops.set_matmul_precision("highest")
        assert ops.f32_compute_code() == _lib.GT_F32 == layers._compute_code()
        ops.set_matmul_precision("high")
        assert ops.f32_compute_code() == _lib.GT_COMPUTE_F32_HIGH == layers._compute_code()
        ops.set_matmul_dtype(torch.bfloat16)   # bf16 matmuls win over the fp32 precision
        assert ops.f32_compute_code() == _lib.GT_BF16 == layers._compute_code()
    finally:
        ops.set_matmul_dtype(torch.float32)
        ops.set_matmul_precision(start)


def test_python_constant_is_the_headers_enum_value():
    from graphtrans_amd import _lib
    src = open(os.path.join(REPO, "include", "graphtrans_hip.h")).read()
    body = re.search(r"enum\s+gt_compute\s*\{([^}]*)\}", src).group(1)
    values = {k: int(v) for k, v in re.findall(r"(GT_COMPUTE_\w+)\s*=\s*(-?\d+)", body)}
    assert values == {"GT_COMPUTE_F32": _lib.GT_F32, "GT_COMPUTE_BF16": _lib.GT_BF16, "GT_COMPUTE_F32_HIGH": _lib.GT_COMPUTE_F32_HIGH}
    assert _lib.GT_COMPUTE_F32_HIGH == 2
    assert "gt_linear_products" in _lib.SIGNATURES and re.search(r"\bint\s+gt_linear_products\s*\(", src)


def test_environment_default_is_read_at_import():
    """GT_F32_PRECISION in a fresh interpreter each (the constant is read once, at import)"""
    code = "from graphtrans_amd import ops; print('precision=' + ops.get_matmul_precision())"
    base = {k: v for k, v in os.environ.items() if k != "GT_F32_PRECISION"}
    base["PYTHONPATH"] = REPO + os.pathsep + base.get("PYTHONPATH", "")
    cases = {None: "highest", "highest": "highest", "high": "high", " High": "high", "medium": None}
    procs = {}
    for val in cases:
        env = dict(base) if val is None else dict(base, GT_F32_PRECISION=val)
        procs[val] = subprocess.Popen([sys.executable, "-c", code], cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    for val, want in cases.items():
        out, err = procs[val].communicate(timeout=300)
        if want is None:
            assert procs[val].returncode != 0 and "GT_F32_PRECISION" in err, (val, out, err[-500:])
        else:
            assert procs[val].returncode == 0 and f"precision={want}" in out, (val, out, err[-500:])
