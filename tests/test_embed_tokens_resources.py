"""Scratch budget of the embed-to-token-row kernels (hipcc -Rpass-analysis=kernel-resource-usage on csrc/embed.hip, no GPU needed),
after tests/test_kernel_resources.py: k_embed_tokens_fwd / k_embed_tokens_dadd for both token types and the three instantiations of
the sorted reduction (node rows, fp32 token rows, bf16 token rows through the row map) use no scratch."""
import re

from test_kernel_resources import _usage


def test_embed_token_kernels_use_no_scratch():
    k = _usage("embed.hip")
    fwd = {n: v for n, v in k.items() if "k_embed_tokens_fwd" in n}
    dadd = {n: v for n, v in k.items() if "k_embed_tokens_dadd" in n}
    reduce_ = {n: v for n, v in k.items() if "k_eseg_reduce" in n}
    assert len(fwd) == 2 and len(dadd) == 2, sorted(k)        # <float>, <gt_bf16>
    assert len(reduce_) == 3, sorted(k)                        # SEG_SRC_NODES, SEG_SRC_TOK_F32, SEG_SRC_TOK_BF16
    assert {re.search(r"ILi(\d)E", n).group(1) for n in reduce_} == {"0", "1", "2"}
    for n, v in {**fwd, **dadd, **reduce_, **{n: v for n, v in k.items() if "k_eseg_fixup" in n}}.items():
        assert "ScratchSize" in v, (n, v)
        assert v["ScratchSize"] == 0, "embed kernel spilling to scratch: %s %s" % (n, v)
