"""GTSFM_MATCH_F16_RERANK reaches 512 dimensions: the binding's constant, the header's text and the workspace the
library asks for (a host-side computation: no GPU needed)."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_max_dim_constant():
    from gtsfm_amd import native

    assert native.GTSFM_MATCH_F16_MAX_DIM == 512


def test_header_documents_512():
    text = open(os.path.join(REPO, "include", "gtsfm_hip.h")).read()
    para = re.search(r"mode GTSFM_MATCH_F16_RERANK:.*?\*/", text, flags=re.S).group(0)
    assert "dim <= 512" in para and "dim > 512 runs" in para and "dim <= 256" not in para
    decl = text.index("int gtsfm_match_rerank_stats(")
    stats = text[text.rindex("/*", 0, decl): decl]  # the comment above the declaration
    assert "dim <= 512" in stats and "dim <= 256" not in stats


def test_workspace_follows_the_512_pad():
    from gtsfm_amd import native

    L = native.lib()
    F16, EXACT = native.GTSFM_MATCH_F16_RERANK, native.GTSFM_MATCH_EXACT_F32
    exact = L.gtsfm_match_workspace_bytes(2, 128, 512, 1, EXACT)
    assert L.gtsfm_match_workspace_bytes(2, 128, 512, 1, F16) > exact > 0
    # 257..512 share the 512-column fp16 operand; past it the request is the exact kernels' again
    assert L.gtsfm_match_workspace_bytes(2, 128, 257, 1, F16) == L.gtsfm_match_workspace_bytes(2, 128, 512, 1, F16)
    assert (L.gtsfm_match_workspace_bytes(2, 128, 512, 1, F16) - L.gtsfm_match_workspace_bytes(2, 128, 256, 1, F16)
            == 2 * 128 * 256 * 2)
    assert L.gtsfm_match_workspace_bytes(2, 128, 513, 1, F16) == L.gtsfm_match_workspace_bytes(2, 128, 513, 1, EXACT)
