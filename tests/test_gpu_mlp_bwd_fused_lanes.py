"""dn_mlp_bwd_fused_bf16 where its lane arithmetic changes path: the row DMAs and result stores from a wave-uniform base (tiles
wholly inside a chunk) against the per-lane path (a chunk's last partial tile and the run-ahead tiles behind it), and the keep
masks from the byte -> word-mask table.  At the launch level, as test_more_chunks_than_one_round_of_workgroups: ops.mlp_bwd_fused
against ops.rows_wgrad (mask_a_bits) + ops.rows_chain2 (mask0_bits, mask1_bits) on ONE chunk table from ops.make_row_chunks, every
result bit for bit, slopes 0 and 1 / 5.5.

A chunk that does not start at a multiple of 32: make_row_chunks([37, n]) gives one (a one-relation table whose rows begin at 37;
the rows in front of it belong to no chunk, so neither side touches them and they are not compared)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = 256
SLOPES = (0.0, 1.0 / 5.5)


def _rand(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(torch.bfloat16).to(DEV)


def _operands(n, seed):
    gen = torch.Generator().manual_seed(seed)
    return dict(g=_rand(gen, n, H), h1=_rand(gen, n, H), x=_rand(gen, n, H), w1=_rand(gen, H, H, scale=1 / 16),
                w2=_rand(gen, H, H, scale=1 / 16),
                bits_in=torch.randint(0, 256, (n, H // 8), generator=gen, dtype=torch.uint8).to(DEV),
                bits_out=torch.randint(0, 256, (n, H // 8), generator=gen, dtype=torch.uint8).to(DEV))


def _every_byte_mask(seed):
    """uint8 [96, 32]: in the rows of each half of a tile (row-in-tile below 16 / from 16 on) every byte value six times, at
    shuffled column positions."""
    gen = torch.Generator().manual_seed(seed)
    m = torch.empty(96, H // 8, dtype=torch.uint8)
    row_in_tile = torch.arange(96) % 32
    for half in (0, 1):
        rows = torch.nonzero((row_in_tile >= 16) == bool(half)).flatten()                   # 48 rows x 32 bytes = 6 x 256
        vals = torch.cat([torch.randperm(256, generator=gen) for _ in range(6)]).to(torch.uint8)
        m[rows] = vals.view(48, H // 8)
        for v in range(256):
            where = torch.nonzero(m[rows] == v)
            assert where.shape[0] == 6 and where[:, 1].unique().numel() >= 2, (half, v)
    return m.to(DEV)


def _same(name, a, b, what=""):
    assert a.dtype == b.dtype and a.shape == b.shape, what + name
    diff = int((a.view(torch.int16) != b.view(torch.int16)).sum())
    assert diff == 0, "%s%s differs in %d elements" % (what, name, diff)


def _both_launches(op, table, slope, first_row=0):
    """((name, fused, reference), ...) of launch A (both masks) and launch B (no masks) against the launches they replace."""
    from dummynode4graphlearning_amd import ops
    with torch.no_grad():
        gw2r, gb2r = ops.rows_wgrad(op["g"], op["h1"], table, 1, colsum_of=1, mask_a_bits=op["bits_in"], colsum_lp=True, slope=slope)
        g1r, g0r = ops.rows_chain2(op["g"], op["w2"], None, False, op["w1"], None, False, mask0_bits=op["bits_in"],
                                   mask1_bits=op["bits_out"], w_kn=(True, True), slope=slope)
        gw1r, gb1r = ops.rows_wgrad(g1r, op["x"], table, 1, colsum_of=1, colsum_lp=True)
        gw2, gb2, g1 = ops.mlp_bwd_fused(op["g"], op["h1"], op["w2"], table, mask_in_bits=op["bits_in"], mask_out_bits=op["bits_out"],
                                         slope=slope)
        gw1, gb1, g0 = ops.mlp_bwd_fused(g1, op["x"], op["w1"], table, slope=slope)
    f = first_row
    return (("gw2", gw2, gw2r[0]), ("gb2", gb2, gb2r[0]), ("g1", g1[f:], g1r[f:]), ("gw1", gw1, gw1r[0]), ("gb1", gb1, gb1r[0]),
            ("g0", g0[f:], g0r[f:]))


def _every_byte_case():
    from dummynode4graphlearning_amd import ops
    op = _operands(96, 11)
    op["bits_in"], op["bits_out"] = _every_byte_mask(21), _every_byte_mask(22)
    return op, ops.make_row_chunks([0, 96], DEV, chunk_rows=128)


@pytest.mark.parametrize("slope", SLOPES)
def test_every_mask_byte_in_both_row_halves(slope):
    op, table = _every_byte_case()
    for name, a, b in _both_launches(op, table, slope):
        _same(name, a, b, "slope=%g: " % slope)


@pytest.mark.parametrize("n", [1, 17, 128 * 3 + 1, 128 * 3 + 16, 128 * 3 + 31, 128 * 3 + 32])
def test_chunk_ends_at_every_residue(n):
    """chunk_rows = 128: full chunks of four whole tiles, then a last chunk of 1 / 16 / 31 / 32 rows (a partial last tile, a full
    last tile, run-ahead tiles wholly past the end); n = 1, 17: a chunk shorter than the ring, the prologue issues tiles past the end."""
    from dummynode4graphlearning_amd import ops
    table = ops.make_row_chunks([0, n], DEV, chunk_rows=128)
    assert table[2] == (n + 127) // 128
    op = _operands(n, 300 + n)
    for slope in SLOPES:
        for name, a, b in _both_launches(op, table, slope):
            _same(name, a, b, "rows=%d slope=%g: " % (n, slope))


def test_chunks_that_start_off_a_tile_boundary():
    from dummynode4graphlearning_amd import ops
    n = 37 + 128 + 50
    table = ops.make_row_chunks([37, n], DEV, chunk_rows=128)
    assert table[2] == 2 and table[0][:, 1].tolist() == [37, 165] and table[0][:, 2].tolist() == [165, n]
    op = _operands(n, 41)
    for slope in SLOPES:
        for name, a, b in _both_launches(op, table, slope, first_row=37):
            _same(name, a, b, "slope=%g: " % slope)


def test_rows_past_two_to_the_23():
    """Row indices whose byte offsets pass 2^32: operands of 2^23 + 200 rows (never initialised but for the last 96), one chunk over
    those 96 rows."""
    from dummynode4graphlearning_amd import ops
    free = torch.cuda.mem_get_info(torch.device(DEV))[0]
    if free < 20 * 2 ** 30:
        pytest.skip("needs 20 GB of free device memory, %.1f GB are free" % (free / 2 ** 30))
    n, tail = 2 ** 23 + 200, 96
    small = _operands(tail, 61)
    op = {k: small[k] for k in ("w1", "w2")}
    for k in ("g", "h1"):
        op[k] = torch.empty(n, H, dtype=torch.bfloat16, device=DEV)
        op[k][n - tail:] = small[k]
    for k in ("bits_in", "bits_out"):
        op[k] = torch.empty(n, H // 8, dtype=torch.uint8, device=DEV)
        op[k][n - tail:] = small[k]
    table = ops.make_row_chunks([n - tail, n], DEV, chunk_rows=128)
    assert table[2] == 1
    try:
        with torch.no_grad():
            for slope in SLOPES:
                gw2r, gb2r = ops.rows_wgrad(op["g"], op["h1"], table, 1, colsum_of=1, mask_a_bits=op["bits_in"], colsum_lp=True,
                                            slope=slope)
                g1r, g0r = ops.rows_chain2(op["g"], op["w2"], None, False, op["w1"], None, False, mask0_bits=op["bits_in"],
                                           mask1_bits=op["bits_out"], w_kn=(True, True), slope=slope)
                g1r = g1r[n - tail:].clone()
                del g0r
                torch.cuda.empty_cache()
                gw2, gb2, g1 = ops.mlp_bwd_fused(op["g"], op["h1"], op["w2"], table, mask_in_bits=op["bits_in"],
                                                 mask_out_bits=op["bits_out"], slope=slope)
                _same("gw2", gw2, gw2r[0], "slope=%g: " % slope)
                _same("gb2", gb2, gb2r[0], "slope=%g: " % slope)
                _same("g1", g1[n - tail:], g1r, "slope=%g: " % slope)
                del g1
                torch.cuda.empty_cache()
    finally:
        op.clear()
        torch.cuda.empty_cache()


def test_every_mask_byte_twice_is_bit_identical():
    op, table = _every_byte_case()
    a = _both_launches(op, table, SLOPES[1])
    b = _both_launches(op, table, SLOPES[1])
    for (name, u, _), (_, v, _) in zip(a, b):
        _same(name, u, v, "second run: ")
