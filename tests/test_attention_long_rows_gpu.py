"""The band-limited (WIN) and packed (SEG) attention kernels on rows of eight and nine 128-row blocks, S = 1024 and 1040, against
float64: a band or a document that starts several blocks below the diagonal block, even and odd first tiles of the forward / dQ
loop, dK/dV sweeps cut short of the row's end, and three batch rows over two kv heads in the dK/dV workgroup split.  Inputs, guarded
outputs and criteria are those of test_attention_window_gpu.py and test_attention_packed_gpu.py."""
import numpy as np
import pytest
import torch

from llm_fp8_amd.pytorch.ops import attn_window_walk
from oracle.fp8_oracle import bf16_bits_to_f32
from tests import test_attention_packed_gpu as P, test_attention_window_gpu as Wn
from tests.test_attention_window_gpu import ops  # noqa: F401  (the fixture)
from tests.util import bf16_bits

pytestmark = pytest.mark.gpu

SHAPES = [(3, 4, 2, 128, True), (2, 2, 1, 64, False)]  # B, H, G, D, fused qkv views; B = 3, G = 2: the dK/dV split lin -> (kbi, g, b)
LENGTHS = [1024, 1040]  # eight full blocks; TAIL: nine, the last of 16 rows


def _ref(q, k, v, do, scale, lo):
    """The arithmetic of _band_ref / _doc_ref under the mask lo[b, i] <= j <= i, one (batch, head) at a time: a few S x S float64
    arrays at once instead of B * H of them -> o, lse (log2 domain), dq, dk, dv."""
    q, k, v, do = (bf16_bits_to_f32(bf16_bits(t)).astype(np.float64) for t in (q, k, v, do))
    B, S, H, D = q.shape
    rep = H // k.shape[2]
    o, dq, dk, dv, lse = np.empty_like(q), np.empty_like(q), np.zeros_like(k), np.zeros_like(k), np.empty((B, H, S))
    j = np.arange(S)
    for b in range(B):
        mask = (lo[b][:, None] <= j) & (j <= j[:, None])
        for h in range(H):
            qh, kh, vh, doh = q[b, :, h], k[b, :, h // rep], v[b, :, h // rep], do[b, :, h]
            s = np.where(mask, np.matmul(qh, kh.T) * scale, -np.inf)
            m = s.max(-1, keepdims=True)
            p = np.exp(s - m)
            l = p.sum(-1, keepdims=True)
            p /= l
            dp = np.matmul(doh, vh.T)
            ds = p * (dp - (p * dp).sum(-1, keepdims=True)) * scale
            o[b, :, h], dq[b, :, h], lse[b, h] = np.matmul(p, vh), np.matmul(ds, kh), (m[:, 0] + np.log(l[:, 0])) / np.log(2.0)
            dk[b, :, h // rep] += np.matmul(ds.T, qh)
            dv[b, :, h // rep] += np.matmul(p.T, doh)
    return o, lse, dq, dk, dv


def _same_bits(first, second):
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), first, second):  # no atomics, no sum across workgroups
        assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16),
                           b.view(torch.int32 if b.dtype == torch.float32 else torch.int16)), f"{name}: two runs differ"


# ------------------------------------------------------------------------------------------------ windows
# 70 and 96: a band inside one block's reach, even first tiles; 129: one key past a block; 300: odd first tiles; 513: the band starts
# four blocks below the diagonal block; 1000: nearly the causal walk, only the last block(s) leave tile 0 out
WINDOWS = [70, 96, 129, 300, 513, 1000]


def test_the_windows_reach_every_walk():
    """ops.attn_window_walk over all blocks of LENGTHS x WINDOWS: the double-buffer parities and both ends of the dK/dV clamp."""
    walks = {(S, W, blk): attn_window_walk(S, W, blk) for S in LENGTHS for W in WINDOWS for blk in range(-(-S // 128))}
    assert attn_window_walk(1040, 100, 2) == (2, 4, 8) and attn_window_walk(1040, 100, 8) == (14, 3, 1)
    band = lambda W: (128 + W - 1 + 31) // 32
    rest = lambda S, blk: -(-S // 32) - 4 * blk
    assert any(j0 > 0 and j0 % 2 == 0 for j0, _, _ in walks.values())
    assert any(j0 % 2 == 1 for j0, _, _ in walks.values())
    assert any(j0 == 0 and blk > 0 for (_, _, blk), (j0, _, _) in walks.items())
    assert any(j0 <= 2 * blk - 4 for (_, _, blk), (j0, _, _) in walks.items())  # the loop starts two blocks or more below the diagonal block
    assert any(n == band(W) < rest(S, blk) for (S, W, blk), (_, _, n) in walks.items())  # the sweep ends with the band, slices left
    assert any(n == rest(S, blk) < band(W) for (S, W, blk), (_, _, n) in walks.items())  # the sweep ends with the row
    for S in LENGTHS:  # and each length has them all by itself
        mine = {key: walk for key, walk in walks.items() if key[0] == S}
        assert any(j0 > 0 and j0 % 2 == 0 for j0, _, _ in mine.values()) and any(j0 % 2 == 1 for j0, _, _ in mine.values())
        assert any(n == band(W) < rest(S, blk) and rest(S, blk) - n >= 8 for (_, W, blk), (_, _, n) in mine.items())  # many slices left


@pytest.mark.parametrize("B,H,G,D,fused", SHAPES)
@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("S", LENGTHS)
def test_window_long_rows_vs_float64(ops, dev, S, W, B, H, G, D, fused):
    q, k, v, do = Wn._inputs(dev, B, S, H, G, D, seed=S + W + D, fused=fused)
    scale = D ** -0.5
    o, lse, dq, dk, dv = Wn._run(ops, q, k, v, do, scale, W)
    lo = np.broadcast_to(np.maximum(np.arange(S) - (W - 1), 0), (B, S))
    Wn._check(o, lse, (dq, dk, dv), _ref(q, k, v, do, scale, lo), v, f"S{S} W{W} B{B} H{H} G{G} D{D}")
    _same_bits((o, lse, dq, dk, dv), Wn._run(ops, q, k, v, do, scale, W))


# ------------------------------------------------------------------------------------------------ documents
def _cuts(name, S):
    """Boundaries of row 0.  Tokens in documents below 16 tokens, which P._check_documents leaves to the whole-tensor check: one for
    "block-ends" at S = 1024 (the document [1023, 1024)), one for "last-token"; rows 1 and 2 add none and one (below)."""
    return {"mid-tile-to-700": [70, 700],                     # starts mid-tile, spans five blocks: late blocks start far below the diagonal
            "every-48": list(range(48, S, 48)),                # aligned to none of 32, 64, 128
            "block-ends": list(range(127, S, 128)),            # the last row of every block begins a document
            "last-token": [1039],                              # a one-token document inside the partial block
            "partial-block": [1024],                           # a document that is exactly the partial block
            "padded-tail": None}[name]                         # cu_seqlens[-1] = 1000 < S


LAYOUTS = [(S, name) for S in LENGTHS for name in ("mid-tile-to-700", "every-48", "block-ends", "padded-tail")] + \
          [(1040, "last-token"), (1040, "partial-block")]


@pytest.mark.parametrize("B,H,G,D,fused", SHAPES)
@pytest.mark.parametrize("S,name", LAYOUTS)
def test_packed_long_rows_vs_float64(ops, dev, S, name, B, H, G, D, fused):
    cuts = _cuts(name, S)
    if cuts is None:  # the rows behind the first are one trailing document each
        cu = [0, 1000]
    else:  # row 1: two documents cut at S / 2 + 8; row 2: a one-token document (of S tokens, the only one below 16), a long one, 16 tokens
        rows = [cuts, [S // 2 + 8], [333, 334, S - 16]]
        cu = [0] + [b * S + c for b in range(B) for c in rows[b] + [S]]
    seg = ops.attn_segments(torch.tensor(cu, dtype=torch.int32, device=dev), B, S)
    q, k, v, do = P._inputs(dev, B, S, H, G, D, seed=S + len(cu) + D, fused=fused)
    got = P._run(ops, q, k, v, do, D ** -0.5, seg)
    ref = _ref(q, k, v, do, D ** -0.5, seg[0].cpu().numpy())
    what = f"S{S} {name} B{B} H{H} G{G} D{D}"
    P._check(got, ref, v, what)
    P._check_documents(got[2:], ref[2:], seg, what)
    _same_bits(got, P._run(ops, q, k, v, do, D ** -0.5, seg))
