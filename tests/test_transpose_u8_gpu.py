"""mi_transpose_u8 against torch's transpose, bit for bit.  distributed.ShardedFP8DP rebuilds every delayed-scaling operand's w8T
with it after each FP8 all-gather (wait_operand), so the backward GEMMs of the sharded mode read nothing else.  Shapes: ragged
ones (one 8 x 8 block, partial 128-tiles both ways, several tiles with partial edges) and every row-sharded operand of Llama-3.2-3B
and Llama-3.1-8B ([N, K] of q|k|v, o, gate|up, down); strided views inside larger buffers with a canary around them; the refusals."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CANARY = 0xA5

RAGGED = [(8, 8), (136, 72), (1000, 264), (4104, 3080)]
# [N, K] of the sharded GEMM weights: 3B (hidden 3072, 24 / 8 heads of 128, ffn 8192), 8B (hidden 4096, 32 / 8 heads, ffn 14336)
OPERANDS_3B = [(5120, 3072), (3072, 3072), (16384, 3072), (3072, 8192)]
OPERANDS_8B = [(6144, 4096), (4096, 4096), (28672, 4096), (4096, 14336)]


@pytest.fixture(scope="module")
def ops(dev):
    from llm_fp8_amd.pytorch import ops as _ops
    from llm_fp8_amd import _lib
    assert _lib.load().mi_device_supported() == 1, "not a gfx950 device"
    return _ops


def _bytes(shape, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)


@pytest.mark.parametrize("R,C", RAGGED + OPERANDS_3B + OPERANDS_8B)
def test_transpose_u8_vs_torch(ops, dev, R, C):
    y = _bytes((R, C), R * 7 + C, dev)
    out = ops.transpose_u8(y)
    assert out.shape == (C, R)
    assert torch.equal(out, y.t()), f"{R}x{C}: {(out != y.t()).sum().item()} bytes differ"
    # into a preallocated [C, R] buffer that holds a canary: every byte is written
    dst = torch.full((C, R), CANARY, dtype=torch.uint8, device=dev)
    ops.transpose_u8(y, out=dst)
    assert torch.equal(dst, y.t())


@pytest.mark.parametrize("R,C", [(8, 8), (136, 72), (1000, 264), (4104, 3080), (3072, 8192)])
def test_transpose_u8_strided_views_leave_the_rest_alone(ops, dev, R, C):
    """ld_y > cols and ld_yT > rows: y a window of a larger source, the output a window of a larger canary-filled destination
    (as w8T is a column block of the operand when a rank finishes its own rows).  Bytes outside the output window stay."""
    src = _bytes((R + 16, C + 24), R + 3 * C, dev)
    y = src[8:8 + R, 16:16 + C]
    big = torch.full((C + 16, R + 40), CANARY, dtype=torch.uint8, device=dev)
    win = big[8:8 + C, 24:24 + R]
    assert y.stride(0) > C and win.stride(0) > R and y.data_ptr() % 8 == 0 and win.data_ptr() % 8 == 0
    src_before = src.clone()
    ops.transpose_u8(y, out=win)
    assert torch.equal(win, y.t())
    outside = torch.ones_like(big, dtype=torch.bool)
    outside[8:8 + C, 24:24 + R] = False
    assert bool((big[outside] == CANARY).all()), f"{int((big[outside] != CANARY).sum())} bytes outside the view were written"
    assert torch.equal(src, src_before)


@pytest.mark.parametrize("R,C", [(0, 64), (64, 0), (0, 0)])
def test_transpose_u8_empty_is_a_no_op(ops, dev, R, C):
    from llm_fp8_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    src = _bytes((64, 64), 1, dev)
    y = src[:R, :C]
    out = ops.transpose_u8(y)
    assert out.shape == (C, R)
    big = torch.full((64, 64), CANARY, dtype=torch.uint8, device=dev)
    ops.transpose_u8(y, out=big[:C, :R])
    assert _lib.load().mi_transpose_u8(src.data_ptr(), big.data_ptr(), R, C, 64, 64, st) == 0  # the C entry: a valid address
    torch.cuda.synchronize()
    assert bool((big == CANARY).all())


def test_transpose_u8_refusals(ops, dev):
    from llm_fp8_amd import _lib
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    src = _bytes((64, 80), 2, dev)
    big = torch.full((80, 64), CANARY, dtype=torch.uint8, device=dev)
    for r, c in [(12, 16), (16, 12), (4, 8), (8, 60)]:  # rows / cols not multiples of 8
        with pytest.raises(RuntimeError, match="multiples of 8"):
            ops.transpose_u8(src[:r, :c], out=big[:c, :r])
    with pytest.raises(RuntimeError, match="multiples of 8"):  # a leading dimension not a multiple of 8
        ops.transpose_u8(torch.zeros((16, 20), dtype=torch.uint8, device=dev)[:, :16], out=big[:16, :16])
    with pytest.raises(RuntimeError, match="aligned"):  # source 4 bytes off an 8-byte boundary
        ops.transpose_u8(src[:16, 4:20], out=big[:16, :16])
    with pytest.raises(RuntimeError, match="aligned"):  # destination 4 bytes off
        ops.transpose_u8(src[:16, :16], out=big[:16, 4:20])
    # the C entry itself: leading dimensions smaller than the extents, negative sizes
    assert lib.mi_transpose_u8(src.data_ptr(), big.data_ptr(), 16, 16, 8, 64, st) != 0
    assert lib.mi_transpose_u8(src.data_ptr(), big.data_ptr(), 16, 16, 80, 8, st) != 0
    assert lib.mi_transpose_u8(src.data_ptr(), big.data_ptr(), -8, 16, 80, 64, st) != 0
    torch.cuda.synchronize()
    assert bool((big == CANARY).all()), "a refused call wrote"
