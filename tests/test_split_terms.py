"""Exact-integer probes of the six split-bf16 products, at every kernel that forms them.

An fp32 operand is split into three bf16 planes x = x0 + x1 + x2, and the six products a_i b_j with i + j <= 2 are
accumulated in fp32 (fd_gemm tiles 4 / 6 / 10 / 12 / 13 / 14, fd_pair_dw, fd_group_dw, the register-chained edge transition;
the split and the product order are defined once, in csrc/fd_split.h, the plane-major order of the two *_dw kernels in
csrc/fd_pair_dw_common.h).
The parity tests of these kernels draw N(0, 1) operands and bound the error by a fraction of the tensor's maximum; a missing
second-order product (2^-17 relative to one term) is about as large as that bound, so they cannot tell whether all six products
are there.  Here the operands are integer-valued fp32 of three classes

  wide  odd integers with 21 significant bits, random sign: all three planes non-zero
  mid   odd integers with 10 significant bits, random sign: two planes, the third is zero
  unit  entries of {-1, 0, +1}: one plane

in three families, one per group of products (A x B, needs (i, j) = planes of A x planes of B):

  1  wide x unit   (0,0) (1,0) (2,0)    7 non-zeros per dot product
  2  unit x wide   (0,0) (0,1) (0,2)    7
  3  mid  x mid    (0,0) (0,1) (1,0) (1,1)    8

Every test asserts its own premises in torch: the third plane of a wide operand is non-zero for at least three quarters of
the elements, the third plane of a mid operand is zero everywhere, the non-zeros hit every 16-wide block of the reduction
index (every k-stage of every kernel is 16 or 32 wide; the ragged last one included), and per output
sum_k (|a0|+|a1|+|a2|) (|b0|+|b1|+|b2|) (+ |what C held|) < 2^24 in units of the result's grid.  Under the last premise every
partial sum, in any order, is an integer below 2^24: the kernel's result must equal the float64 product BIT FOR BIT
(torch.equal), and a dropped or misindexed product changes almost every output.  One case per family scales the operands by
powers of two (A 2^-30, B 2^+12): exactness is unchanged, the exponent handling of the split is exercised.  Where a kernel
transposes its operands the families run in both role orders.  fd_gemm tile 1 (fp32 MFMA, no split) runs the same probes as
the control: a failure there is a failure of the probe.

In the edge transition the family reaches one layer at a time: the other layers are signed selection matrices (one +-2^e per
output), so the activation that reaches the probed layer is a chosen class; ReLU zeroes the negative units and the result
stays exact.  Checked: the saves h1, h2 + [z|0|0], the pre-LayerNorm y (forward) and d2, d1, dz (backward, gate masks taken
from a forward whose units are all clearly positive or negative).  The LayerNorm outputs are not exact and not part of this.

Achieved: every case exact under the interpreter and on an MI355X (the GPU tier records the number of inexact outputs per
site through parity_log: 0) -- the bf16 MFMA accumulates these integers exactly.  The first GPU run found tile 12 with
row-contiguous weights inexact in family 1 (1,000 - 2,900 outputs per launch, errors <= 30 at results of ~4e6, varying from
launch to launch): a v_cvt_pk_bf16_f32 inside an asm statement one wait state in front of the MFMA reading its result; fixed in
csrc/gfx950/fd_intrin.h (pack_bf16), see DESIGN.md, Numerics.

Left out on purpose:
  * the column-split inference kernel (edge_shape=2): it exposes post-LayerNorm outputs only, and test_edge_mlp ties it to
    shape 4 within 3e-6;
  * the edge embedder: its inputs are computed features, not free matrices; its measured bound caught a removed product;
  * the attention kernels: a softmax sits between the products;
  * fd_gemm tiles 2, 3, 5 and fd_ln_gemm: fp32 MFMA, no split.
"""
import pytest
import torch

import parity_log
from se3_diffusion_amd import ops, options

LIM = float(2 ** 24)
# family -> (class of A, class of B, which operand is sparse, non-zeros per dot product)
FAMILIES = {1: ("wide", "unit", "B", 7), 2: ("unit", "wide", "A", 7), 3: ("mid", "mid", "B", 8)}
EA, EB = -30, 12                      # the scaled cases: A 2^-30, B 2^+12
_INEXACT = {}                         # (tier, site) -> outputs that differ from the exact result (expected 0), for parity_log


# ---------------------------------------------------------------------------------------------------------------------
# operand classes and premises
# ---------------------------------------------------------------------------------------------------------------------
def _sign(g, shape):
    return (1 - 2 * torch.randint(0, 2, shape, generator=g)).float()


def dense(g, cls, *shape, signed=True):
    """a dense operand of a class; signed=False: the non-negative half of the class (passes a ReLU unchanged)"""
    if cls == "wide":
        v = (2 * torch.randint(2 ** 19, 2 ** 20, shape, generator=g) + 1).float()          # odd, 2^20 < v < 2^21
    elif cls == "mid":
        v = (2 * torch.randint(2 ** 8, 2 ** 9, shape, generator=g) + 1).float()            # odd, 2^9 < v < 2^10
    else:
        v = (torch.rand(shape, generator=g) < 0.75).float()                                 # {0, 1}, three quarters set
    return v * _sign(g, shape) if signed else v


def sparse(g, cls, K, n, nnz):
    """[K, n]: every column (= every dot product) has nnz non-zeros of the class at random reduction indices.  The 16-wide k
    blocks are dealt out from shuffled decks, column after column, so that a few columns already reach every block (the ragged
    last one included); the index inside a block is random.  (Two picks of a column may coincide: nnz is an upper bound.)"""
    nblk = (K + 15) // 16
    decks = (n * nnz + nblk - 1) // nblk
    blk = torch.cat([torch.randperm(nblk, generator=g) for _ in range(decks)])[:n * nnz].view(n, nnz)
    width = torch.clamp(K - 16 * blk, max=16)
    idx = 16 * blk + torch.randint(0, 16, (n, nnz), generator=g) % width
    mask = torch.zeros(n, K).scatter_(1, idx, 1.0).t()
    v = _sign(g, (K, n)) if cls == "unit" else dense(g, cls, K, n)
    return (v * mask).contiguous()


def operands(g, fam, M, N, K, swap=False):
    """A [M, K], B [K, N] of a family; swap: the classes (and the sparse side) change operands"""
    ca, cb, side, nnz = FAMILIES[fam]
    if swap:
        ca, cb, side = cb, ca, "A" if side == "B" else "B"
    if side == "B":
        A, B = dense(g, ca, M, K), sparse(g, cb, K, N, nnz)
    else:
        A, B = sparse(g, ca, K, M, nnz).t().contiguous(), dense(g, cb, K, N)
    return A, B, (ca, cb)


def planes(x):
    """the three round-to-nearest bf16 terms of an fp32 tensor (exact: x0 + x1 + x2 == x)"""
    x0 = x.bfloat16().float()
    r = x - x0
    x1 = r.bfloat16().float()
    x2 = (r - x1).bfloat16().float()
    assert torch.equal((x0.double() + x1.double() + x2.double()), x.double())
    return x0, x1, x2


def _is_class(x, cls):
    """premise: the planes of x are those of its class (x in integer units)"""
    assert torch.equal(x, x.round()), "integer-valued"
    p0, p1, p2 = planes(x)
    nz = x != 0
    assert bool(nz.any())
    if cls == "wide":
        share = float((p2[nz] != 0).float().mean())
        assert share >= 0.75, ("third plane of a wide operand", share)
    elif cls in ("mid", "mid+"):
        assert not bool(p2.any()), "third plane of a mid operand"
        # (mid+: sums of two mid numbers -- 11 bits or fewer, still no third plane)
        assert cls == "mid+" or bool((p1[nz] != 0).all()), "second plane of a mid operand"
    else:
        assert not bool(p1.any()) and not bool(p2.any()), "unit operand: one plane"


def _wide_share(x):
    """share of ALL elements of a dense wide operand whose third plane is non-zero"""
    return float((planes(x)[2] != 0).float().mean())


def _abs_planes(x):
    p0, p1, p2 = planes(x)
    return p0.double().abs() + p1.double().abs() + p2.double().abs()


def premises(A, B, classes, sa=1.0, sb=1.0, extra=None):
    """A [M, K] (scale sa), B [K, N] (scale sb), extra [M, N]: |what is added to the product| -- asserts the classes, the k-stage
    coverage and the 2^24 budget; returns the exact result (float64)"""
    Ai, Bi = (A.double() / sa).float(), (B.double() / sb).float()
    assert torch.equal(Ai.double() * sa, A.double()) and torch.equal(Bi.double() * sb, B.double())
    _is_class(Ai, classes[0])
    _is_class(Bi, classes[1])
    for x, cls in ((Ai, classes[0]), (Bi, classes[1])):
        if cls == "wide" and bool((x != 0).float().mean() > 0.5):            # a dense wide operand: share of all elements
            assert _wide_share(x) >= 0.75
    # scaled planes = planes of the integers x the scale (the split commutes with powers of two)
    if sa != 1.0:
        assert all(torch.equal(p.double() * sa, q.double()) for p, q in zip(planes(Ai), planes(A)))
    if sb != 1.0:
        assert all(torch.equal(p.double() * sb, q.double()) for p, q in zip(planes(Bi), planes(B)))
    K = A.shape[1]
    hit = (Ai != 0).any(0) & (Bi != 0).any(1)                                  # reduction indices some output's product hits
    pad = torch.zeros((-K) % 16, dtype=torch.bool)
    blocks = torch.cat([hit, pad]).view(-1, 16).any(1)
    assert bool(blocks.all()), ("a 16-wide k block without a non-zero product", blocks.tolist())
    budget = _abs_planes(Ai) @ _abs_planes(Bi)
    if extra is not None:
        budget = budget + extra.double().abs() / (sa * sb)
    assert float(budget.max()) < LIM, ("2^24 budget", float(budget.max()))
    ref = A.double() @ B.double()
    return ref


def _exact(site, got, ref, what="", tier=None):
    """got (fp32, any device) == ref (float64, exactly representable) bit for bit; the count of differing outputs is kept"""
    r32 = ref.float()
    assert torch.equal(r32.double(), ref), "the reference is an fp32 number"
    bad = int((got.detach().cpu() != r32).sum())
    key = (tier or ("gpu" if got.is_cuda else "emu"), site)
    _INEXACT[key] = _INEXACT.get(key, 0) + bad           # (kept before the assertion: a failing run records its count)
    assert bad == 0 and torch.equal(got.detach().cpu(), r32), (site, what, f"{bad} of {r32.numel()} outputs inexact")


class _logged:
    """GPU tier: on leaving the block -- passed or failed -- record the inexact outputs of the sites it ran through parity_log"""

    def __init__(self, *sites):
        self.sites = sites

    def __enter__(self):
        for site in self.sites:
            _INEXACT[("gpu", site)] = 0

    def __exit__(self, et, ev, tb):
        for site in self.sites:
            try:
                with parity_log.case(f"split_terms_{site}"):
                    parity_log.out("inexact_outputs", _INEXACT[("gpu", site)])
                    assert et is None
            except AssertionError:
                pass                                      # (the case is recorded as failed; the test's own error goes on)
        return False


def _sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


def _small_ints(g, *shape, lim=50):
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


# ---------------------------------------------------------------------------------------------------------------------
# 1. fd_gemm tiles 4, 6, 10 (tile 1: the fp32-MFMA control)
# ---------------------------------------------------------------------------------------------------------------------
SPLIT_LAYOUTS = [(True, True), (True, False), (False, False)]
ALL_LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]
TILE_LAYOUTS = {1: ALL_LAYOUTS, 4: SPLIT_LAYOUTS, 6: SPLIT_LAYOUTS, 10: ALL_LAYOUTS}


def _gemm(lib, dev, tile, a_kc, b_kc, fam, M, N, K, seed, scaled=False, ksplit=1, persistent=0):
    g = torch.Generator().manual_seed(seed)
    A, B, classes = operands(g, fam, M, N, K)
    sa, sb = (2.0 ** EA, 2.0 ** EB) if scaled else (1.0, 1.0)
    A, B = A * sa, B * sb
    C0 = _small_ints(g, M, N) * (sa * sb)                 # C accumulates: non-zero integers on the result's grid
    ref = premises(A, B, classes, sa, sb, extra=C0) + C0.double()
    if a_kc:
        At, a_str = A.contiguous(), (K, 1)
    else:
        At, a_str = A.t().contiguous(), (1, M)            # stored [K][M]
    if b_kc:
        Bt, b_str = B.t().contiguous(), (1, K)            # stored W[N][K]
    else:
        Bt, b_str = B.contiguous(), (N, 1)
    C = C0.clone().to(dev)
    was = lib.cdll.fd_gemm_set_persistent_blocks(persistent) if persistent else None
    try:
        if persistent:
            # the persistent kernel (its own copy of the product table) runs from two 256 x 128 tiles per block up, on the
            # k-contiguous-A layouts without split-K: the case must be on that side of the rule, and the setter must have taken
            assert lib.cdll.fd_gemm_set_persistent_blocks(persistent) == persistent
            assert tile == 4 and a_kc and ksplit == 1 and ((M + 255) // 256) * ((N + 127) // 128) >= 2 * persistent
        # (split-K adds its partial tiles into C; one pass accumulates with beta)
        lib.gemm(At.to(dev), Bt.to(dev), C, M, N, K, a_str, b_str, N, tile=tile, ksplit=ksplit, beta=(ksplit == 1))
        _sync(dev)
    finally:
        if persistent:
            lib.cdll.fd_gemm_set_persistent_blocks(was)
    _exact(f"gemm_tile{tile}", C, ref, (a_kc, b_kc, fam, M, N, K, scaled, ksplit, persistent))


def _gemm_site(lib, dev, tile, fam):
    # 200 = 12 stages of 16 + a ragged one of 8 (tile 10: 6 of 32 + 8); 300 x 136: more than one block in M and N on every tile
    for n, (a_kc, b_kc) in enumerate(TILE_LAYOUTS[tile]):
        _gemm(lib, dev, tile, a_kc, b_kc, fam, 100, 72, 200, seed=10 * fam + n)
    a_kc, b_kc = TILE_LAYOUTS[tile][0]
    _gemm(lib, dev, tile, a_kc, b_kc, fam, 300, 136, 200, seed=10 * fam + 5)
    _gemm(lib, dev, tile, a_kc, b_kc, fam, 100, 72, 200, seed=10 * fam + 6, scaled=True)
    _gemm(lib, dev, tile, False, False, fam, 100, 72, 200, seed=10 * fam + 7, ksplit=3)        # dW-like, as ops launches it
    if tile == 4:
        # persistent blocks of the wide kernel: 2 x 2 tiles of 256 x 128 on 2 blocks, each block walks two tiles
        _gemm(lib, dev, tile, True, True, fam, 300, 136, 200, seed=10 * fam + 8, persistent=2)
        _gemm(lib, dev, tile, True, False, fam, 300, 136, 200, seed=10 * fam + 9, persistent=2)


@pytest.mark.parametrize("fam", [1, 2, 3])
@pytest.mark.parametrize("tile", [1, 4, 6, 10])
def test_gemm_terms_emu(emu_lib, tile, fam):
    _gemm_site(emu_lib, "cpu", tile, fam)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [1, 4, 6, 10])
def test_gemm_terms_gpu(hip_lib, tile):
    with _logged(f"gemm_tile{tile}"):
        for fam in (1, 2, 3):
            _gemm_site(hip_lib, "cuda", tile, fam)


# ---------------------------------------------------------------------------------------------------------------------
# 2. fd_gemm tiles 12, 13, 14: activations x weights pre-split by fd_split_planes
# ---------------------------------------------------------------------------------------------------------------------
def _planes_of(lib, buf):
    n = buf.numel()
    assert n % 8 == 0
    pl = torch.empty((3, n), dtype=torch.int16, device=buf.device)
    lib.call("fd_split_planes", buf, n, pl)
    return pl


def _gemm_w(lib, dev, tile, b_kc, fam, M, N, K, seed, sub=False, scaled=False, ksplit=1):
    g = torch.Generator().manual_seed(seed)
    A, B, classes = operands(g, fam, M, N, K)
    sa, sb = (2.0 ** EA, 2.0 ** EB) if scaled else (1.0, 1.0)
    A, B = A * sa, B * sb
    C0 = _small_ints(g, M, N) * (sa * sb)
    ref = premises(A, B, classes, sa, sb, extra=C0) + C0.double()
    Wn, Wk = (N, K) if b_kc else (K, N)                   # y = x W^T: W [N, K]; dx = dy W: W [K, N]
    # the weight sits inside a larger flat parameter buffer at an offset, optionally as a column block of a wider matrix
    ld = Wk + (24 if sub else 0)
    off = 64 + (8 if sub else 0)
    flat = dense(g, "wide", off + Wn * ld + 64) * sb      # (what surrounds the weight must not leak into the product)
    flat[off:off + Wn * ld].view(Wn, ld)[:, :Wk] = B.t() if b_kc else B
    flat_d, C = flat.to(dev), C0.clone().to(dev)
    pl = _planes_of(lib, flat_d)
    b_str = (1, ld) if b_kc else (ld, 1)
    lib.gemm(A.to(dev), flat_d, C, M, N, K, (K, 1), b_str, N, b_off=off, tile=tile, ksplit=ksplit, beta=(ksplit == 1),
             b_planes=(pl.data_ptr() + 2 * off, flat.numel()))
    _sync(dev)
    _exact(f"gemm_w_tile{tile}", C, ref, (b_kc, fam, M, N, K, sub, scaled, ksplit))


def _gemm_w_site(lib, dev, tile, fam):
    # ragged M and N (N a multiple of 8), K = 208: 13 stages of 16 -- the ring wraps several times
    for n, b_kc in enumerate((True, False)):
        _gemm_w(lib, dev, tile, b_kc, fam, 100, 72, 208, seed=100 + 10 * fam + n)
        _gemm_w(lib, dev, tile, b_kc, fam, 130, 136, 208, seed=100 + 10 * fam + 2 + n, sub=True)
    _gemm_w(lib, dev, tile, True, fam, 100, 72, 208, seed=100 + 10 * fam + 4, scaled=True)
    _gemm_w(lib, dev, tile, False, fam, 100, 72, 208, seed=100 + 10 * fam + 5, sub=True, scaled=True)
    # split-K: the row-major accumulation, both weight layouts
    _gemm_w(lib, dev, tile, True, fam, 70, 40, 208, seed=100 + 10 * fam + 6, ksplit=3)
    _gemm_w(lib, dev, tile, False, fam, 70, 40, 208, seed=100 + 10 * fam + 7, ksplit=3)


@pytest.mark.parametrize("fam", [1, 2, 3])
@pytest.mark.parametrize("tile", [12, 13, 14])
def test_gemm_w_terms_emu(emu_lib, tile, fam):
    _gemm_w_site(emu_lib, "cpu", tile, fam)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [12, 13, 14])
def test_gemm_w_terms_gpu(hip_lib, tile):
    with _logged(f"gemm_w_tile{tile}"):
        for fam in (1, 2, 3):
            _gemm_w_site(hip_lib, "cuda", tile, fam)


# ---------------------------------------------------------------------------------------------------------------------
# 3. fd_pair_dw: C[m, n] += sum_p A[p, m] B[p, n], the pair row p is the reduction index
# ---------------------------------------------------------------------------------------------------------------------
def _colsum_check(site, got, A, c0, scale, rows):
    """the bias gradient (column sums of A, plain fp32 adds -- not a split product): exact where the sum of magnitudes stays below
    2^24, else within the fp32 summation bound rows * 2^-24 * sum |a|"""
    want = c0.double() + A.double().sum(0)
    mag = (c0.double().abs() + A.double().abs().sum(0)) / scale
    tier = "gpu" if got.is_cuda else "emu"
    got = got.detach().cpu().double()
    ok = mag < LIM
    _exact(site, got[ok].float(), want[ok], "colsum", tier=tier)
    assert bool(((got - want).abs() <= rows * 2.0 ** -24 * mag * scale).all()), (site, "colsum bound")


def _dw_pair(g, fam, swap, rows, m, n, sa, sb):
    """dY [rows, m] (scale sa), X [rows, n] (scale sb) of a family and the exact dY^T X"""
    A, B, classes = operands(g, fam, m, n, rows, swap=swap)
    return (A.t().contiguous() * sa), B * sb, classes


def _pair_dw(dev, fam, swap, rows, blocks, seed, scaled=False, lda=384):
    g = torch.Generator().manual_seed(seed)
    sa, sb = (2.0 ** EA, 2.0 ** EB) if scaled else (1.0, 1.0)
    q = sa * sb
    d2, h1, c_w2 = _dw_pair(g, fam, swap, rows, 384, 384, sa, sb)
    d1, z, c_w1 = _dw_pair(g, fam, swap, rows, 384, 128, sa, sb)
    hs, dy, c_wf = _dw_pair(g, fam, swap, rows, 384, 128, sa, sb)        # hs = h2 + [z_add | 0 | 0], the staged operand
    z_add = _small_ints(g, rows, 128, lim=5) * sa
    h2 = hs.clone()
    h2[:, :128] -= z_add                                                 # (exact: integers far below 2^24)
    assert torch.equal(h2[:, :128] + z_add, hs[:, :128])
    C0 = dict(gW2=_small_ints(g, 384, 384) * q, gb2=_small_ints(g, 384) * sa, gW1=_small_ints(g, 384, 384) * q,
              gWf=_small_ints(g, 128, 384) * q)
    rW2 = premises(d2.t(), h1, c_w2, sa, sb, extra=C0["gW2"]) + C0["gW2"].double()
    rW1 = C0["gW1"].double().clone()
    rW1[:, :128] += premises(d1.t(), z, c_w1, sa, sb, extra=C0["gW1"][:, :128])
    rWf = premises(hs.t(), dy, c_wf, sa, sb, extra=C0["gWf"].t()).t() + C0["gWf"].double()
    if lda > 384:                                                        # A = a column slice of a wider tensor
        wide_t = dense(g, "wide", rows, lda) * sa
        wide_t[:, 64:448] = d2
        d2d = wide_t.to(dev)[:, 64:448]
    else:
        d2d = d2.to(dev)
    t = {k: v.to(dev) for k, v in dict(h1=h1, d1=d1, z=z, h2=h2, dy=dy, z_add=z_add).items()}
    G = {k: v.clone().to(dev) for k, v in C0.items()}
    d2v = (d2d, 0, d2d.stride(0))
    items = [dict(A=d2v, B=(t["h1"], 128 * j, 384), C=(G["gW2"], 128 * j, 384), colsum=G["gb2"] if j == 0 else None)
             for j in range(3)]
    items.append(dict(A=(t["d1"], 0, 384), B=(t["z"], 0, 128), C=(G["gW1"], 0, 384)))
    items.append(dict(A=(t["h2"], 0, 384), A_add=(t["z_add"], 0, 128), B=(t["dy"], 0, 128), C=(G["gWf"], 0, 384), trans=True))
    ops.pair_dw(items, rows, blocks=blocks)
    _sync(dev)
    what = (fam, swap, rows, blocks, scaled, lda)
    _exact("pair_dw", G["gW2"], rW2, ("W2",) + what)
    _exact("pair_dw", G["gW1"], rW1, ("W1",) + what)                      # (columns 128.. belong to other launches: untouched)
    _exact("pair_dw", G["gWf"], rWf, ("Wf",) + what)
    _colsum_check("pair_dw", G["gb2"], d2, C0["gb2"], sa, rows)


def _pair_dw_narrow(dev, fam, swap, rows, blocks, seed):
    """a_bands = 1 (A [rows, 128]: a 128 x 128 tile) and b_cols = 120 -- the launch of the edge embedder's layers"""
    g = torch.Generator().manual_seed(seed)
    shapes = ((128, 128), (128, 128), (128, 120))
    items, checks = [], []
    for m, n in shapes:
        A, B, classes = _dw_pair(g, fam, swap, rows, m, n, 1.0, 1.0)
        C0, b0 = _small_ints(g, m, n), _small_ints(g, m)
        ref = premises(A.t(), B, classes, extra=C0) + C0.double()
        Ad, Bd, Cd, bd = A.to(dev), B.to(dev), C0.clone().to(dev), b0.clone().to(dev)
        items.append(dict(A=(Ad, 0, m), B=(Bd, 0, n), C=(Cd, 0, n), colsum=bd, a_bands=1, **(dict(b_cols=n) if n != 128 else {})))
        checks.append((Cd, ref, bd, A, b0))
    ops.pair_dw(items, rows, blocks=blocks)
    _sync(dev)
    for Cd, ref, bd, A, b0 in checks:
        _exact("pair_dw_narrow", Cd, ref, (fam, swap, rows, blocks))
        _colsum_check("pair_dw_narrow", bd, A, b0, 1.0, rows)


def _pair_dw_site(dev, fam):
    for swap in (False, True):                                            # (the trans item multiplies B x A: both role orders)
        _pair_dw(dev, fam, swap, rows=150, blocks=8, seed=200 + 10 * fam + swap)        # one group: 9 full stages + a ragged one
        _pair_dw_narrow(dev, fam, swap, rows=150, blocks=8, seed=220 + 10 * fam + swap)
    _pair_dw(dev, fam, False, rows=150, blocks=16, seed=204 + 10 * fam)                 # three row ranges add into C
    _pair_dw(dev, fam, True, rows=150, blocks=8, seed=205 + 10 * fam, scaled=True)
    _pair_dw(dev, fam, False, rows=90, blocks=8, seed=206 + 10 * fam, lda=512)


@pytest.mark.parametrize("fam", [1, 2, 3])
def test_pair_dw_terms_emu(use_emu, fam):
    _pair_dw_site("cpu", fam)


@pytest.mark.gpu
def test_pair_dw_terms_gpu(hip_lib):
    with _logged("pair_dw", "pair_dw_narrow"):
        for fam in (1, 2, 3):
            _pair_dw_site("cuda", fam)
            _pair_dw("cuda", fam, False, rows=300, blocks=0, seed=207 + 10 * fam)       # the launch's own block count


# ---------------------------------------------------------------------------------------------------------------------
# 4. fd_group_dw through ops.queue_dw / flush_dw
# ---------------------------------------------------------------------------------------------------------------------
GROUP_SHAPES = [(320, 320, True), (200, 132, False), (4, 8, True), (136, 4, True)]      # of test_group_dw.SHAPES_SMALL


def _group_dw(dev, fam, swap, rows, shapes, blocks, seed, slices=True, scaled=False):
    g = torch.Generator().manual_seed(seed)
    sa, sb = (2.0 ** EA, 2.0 ** EB) if scaled else (1.0, 1.0)
    items = []
    for i, (n, k, bias) in enumerate(shapes):
        pad_a, pad_b, pad_c = (8, 8, 12) if (slices and i % 2 == 0) else (0, 0, 0)
        oa, ob, oc = pad_a // 2, pad_b // 2, pad_c // 3                    # float4-addressable column slices
        dY, X, classes = _dw_pair(g, fam, swap, rows, n, k, sa, sb)
        A = dense(g, "wide", rows, n + pad_a) * sa
        A[:, oa:oa + n] = dY
        Bm = dense(g, "wide", rows, k + pad_b) * sb
        Bm[:, ob:ob + k] = X
        C0 = _small_ints(g, n, k + pad_c) * (sa * sb)
        b0 = _small_ints(g, n) * sa if bias else None
        want = C0.double().clone()
        want[:, oc:oc + k] += premises(dY.t(), X, classes, sa, sb, extra=C0[:, oc:oc + k])
        items.append((A.to(dev), oa, Bm.to(dev), ob, C0.clone().to(dev), oc, None if b0 is None else b0.clone().to(dev), n, k,
                      want, dY, b0))
    with options.override(grouped_node_dw=True):
        for A, oa, Bm, ob, C, oc, db, n, k, *_ in items:
            assert ops.queue_dw((A, oa, A.shape[1]), (Bm, ob, Bm.shape[1]), (C, oc, C.shape[1]), rows, n, k, db=db)
        ops.flush_dw(blocks=blocks)
        ops.join_grad_stream()
    _sync(dev)
    for A, oa, Bm, ob, C, oc, db, n, k, want, dY, b0 in items:
        _exact("group_dw", C, want, (fam, swap, rows, n, k, blocks, scaled))    # (the pad columns of C included: untouched)
        if db is not None:
            _colsum_check("group_dw", db, dY, b0, sa, rows)


def _group_dw_site(dev, fam):
    for swap in (False, True):
        _group_dw(dev, fam, swap, 150, GROUP_SHAPES, blocks=3, seed=300 + 10 * fam + swap)     # many units per block, ragged stage
    _group_dw(dev, fam, False, 300, [(132, 260, True)], blocks=2, seed=303 + 10 * fam, slices=False)   # row ranges (nsplit > 1)
    _group_dw(dev, fam, True, 150, GROUP_SHAPES[:2], blocks=3, seed=304 + 10 * fam, scaled=True)


@pytest.mark.parametrize("fam", [1, 2, 3])
def test_group_dw_terms_emu(use_emu, fam):
    _group_dw_site("cpu", fam)


@pytest.mark.gpu
def test_group_dw_terms_gpu(hip_lib):
    with _logged("group_dw"):
        for fam in (1, 2, 3):
            _group_dw_site("cuda", fam)
            _group_dw("cuda", fam, False, 300, GROUP_SHAPES, blocks=0, seed=305 + 10 * fam)    # the launch's own block count


# ---------------------------------------------------------------------------------------------------------------------
# 5 / 6. fd_edge_mlp, shapes 4 and 8: the register-chained products, one layer at a time
# ---------------------------------------------------------------------------------------------------------------------
def selection(g, n_out, n_in, scale=1.0, neg=1.0 / 16, src=None):
    """[n_out, n_in]: one +-scale per row (a signed selection of the inputs; `neg` of the rows negative), drawn from the input
    columns `src` (default: all) so that every one of them is selected about equally often"""
    src = torch.arange(n_in) if src is None else src
    pick = src[torch.randperm(len(src), generator=g)].repeat((n_out + len(src) - 1) // len(src))[:n_out]
    pick = pick[torch.randperm(n_out, generator=g)]
    W = torch.zeros(n_out, n_in)
    W[torch.arange(n_out), pick] = torch.where(torch.rand(n_out, generator=g) < neg, -scale, scale)
    return W


def _pair_index(B, N):
    qi = torch.arange(B * N * N) // N
    qj = (qi // N) * N + torch.arange(B * N * N) % N
    return qi, qj


def _fits(x, q, what):
    """premise of an intermediate result: a multiple of q below 2^24 q (an exact fp32 number, whatever the order of its adds)"""
    assert torch.equal((x / q).round(), x / q) and float(x.abs().max()) < LIM * q, what


def _edge_fwd(dev, layer, fam, shape, B, N, blocks, seed, scaled=False):
    """forward probe of layer 1 / 2 / f(inal): the family's A is the activation that reaches the layer, its B the layer's weight
    (the sparse side: 7 or 8 non-zeros per output unit); the other layers are signed selections"""
    g = torch.Generator().manual_seed(seed)
    ca, cb, _, nnz = FAMILIES[fam]
    R, P = B * N, B * N * N
    sa, sb = (2.0 ** EA, 2.0 ** EB) if scaled else (1.0, 1.0)
    qi, qj = _pair_index(B, N)
    # z: channels 64.. carry random signs; 0..63 are non-negative and feed the trunk (they pass its ReLUs unchanged)
    z = dense(g, ca, P, 128, signed=False)
    if layer == "1":
        z = z * _sign(g, (P, 128))
    else:
        z[:, 64:] *= _sign(g, (P, 64))
    z = z * sa
    trunk_src = None if layer == "1" else torch.arange(64)
    target = lambda n_out, k: sparse(g, cb, k, n_out, nnz).t().contiguous() * sb       # W [n_out, k]
    W1 = torch.zeros(384, 384)
    if layer == "1":
        W1[:, :128] = target(384, 128)
        W2, Wf = selection(g, 384, 384, 1.0 / sb), selection(g, 128, 384)
        q1, q2, qf = sa * sb, sa, sa
    elif layer == "2":
        W1[:, :128] = selection(g, 384, 128, src=trunk_src)
        W2, Wf = target(384, 384), selection(g, 128, 384, 1.0 / sb)
        if scaled:
            W2[:128] = 0.0                        # h2 + [z|0|0] adds numbers of two grids otherwise
        q1, q2, qf = sa, sa * sb, sa / sb if scaled else sa
    else:
        W1[:, :128] = selection(g, 384, 128, src=trunk_src)
        # (the k-stage coverage premise puts non-zeros of Wf on all 24 k blocks: columns 0..127, the z residual part of the
        #  final layer's input, and the h2 part)
        W2, Wf = selection(g, 384, 384), target(128, 384)
        if fam != 3:
            W2[:128] = 0.0                        # columns 0..127 of h2 + [z|0|0] are z: the signed part of the class
        q1, q2, qf = sa, sa, sa * sb
    W1[:, 128:] = dense(g, "wide", 384, 256)      # (the e_i / e_j columns: P1 / Q1 carry them; must not leak in)
    bias = (lambda *s: torch.zeros(*s)) if scaled else (lambda *s: _small_ints(g, *s, lim=3))
    zero = lambda *s: torch.zeros(*s)
    # (a bias in front of the probed layer would change the class of the activation that reaches it)
    b_1, b_2 = (bias if layer == "1" else zero), (bias if layer in "12" else zero)
    P1, Q1, b2, Pf, Qf = b_1(R, 384) * q1, b_1(R, 384) * q1, b_2(384) * q2, bias(R, 128) * qf, bias(R, 128) * qf
    gamma, beta = 1 + 0.2 * torch.randn(128, generator=g), 0.2 * torch.randn(128, generator=g)
    # ---- the exact chain (float64) and the premises of every step
    zd = z.double()
    pq1 = (P1[qi] + Q1[qj]).double()
    pre1 = zd @ W1[:, :128].double().t() + pq1
    h1 = torch.relu(pre1)
    pre2 = h1 @ W2.double().t() + b2.double()
    h2 = torch.relu(pre2)
    h2z = h2.clone()
    h2z[:, :128] += zd
    pqf = (Pf[qi] + Qf[qj]).double()
    y = h2z @ Wf.double().t() + pqf
    if bool(h2[:, :128].any()):
        _fits(h2[:, :128].abs() + zd.abs(), sa, "h2 + z")
    steps = {"1": (z, W1[:, :128], pq1, pre1, q1), "2": (h1.float(), W2, b2.double().expand(P, 384), pre2, q2),
             "f": (h2z.float(), Wf, pqf, y, qf)}
    for L, (x, W, add, res, q) in steps.items():
        assert torch.equal(x.double(), {"1": zd, "2": h1, "f": h2z}[L])                      # an fp32 number
        if L == layer:
            # (final layer, family 3: columns 0..127 of its input are sums of two mid numbers)
            cls = ("mid+", cb) if (layer == "f" and fam == 3) else (ca, cb)
            assert torch.equal(premises(x, W.t().contiguous(), cls, sa, sb, extra=add) + add, res)
        else:
            # a selection layer: one product per output (every plane of the activation times +-2^e), plus the bias
            assert int((W != 0).sum(1).max()) <= 1
            assert torch.equal((res - add).float().double(), res - add)
            if bool(add.any()):
                _fits((res - add).abs() + add.abs(), q, ("selection layer", L))
    # ---- the kernel
    t = {k: v.to(dev) for k, v in dict(z=z, P1=P1, Q1=Q1, b2=b2, Pf=Pf, Qf=Qf, W1=W1, W2=W2, Wf=Wf, gamma=gamma, beta=beta).items()}
    e = lambda *s: torch.full(s, float("nan"), device=dev)
    out, s1, s2, yk, mean, rstd = e(P, 128), e(P, 384), e(P, 384), e(P, 128), e(P), e(P)
    m1 = torch.zeros(P, 12, dtype=torch.int32, device=dev)
    m2 = torch.zeros(P, 12, dtype=torch.int32, device=dev)
    with options.override(edge_shape=shape):
        img = ops.edge_mlp_pack(t["W1"], t["W2"], t["Wf"])
        ops.edge_mlp(t["z"], img, out, P, N, p1=t["P1"], q1=t["Q1"], bias2=t["b2"], pf=t["Pf"], qf=t["Qf"], gamma=t["gamma"],
                     beta=t["beta"], rowscale=torch.ones(P, device=dev), save1=s1, save2=s2, y=yk, mean=mean, rstd=rstd,
                     blocks=blocks, mask1=m1, mask2=m2)
    _sync(dev)
    site = f"edge_mlp_fwd_w{shape}"
    what = (layer, fam, B, N, blocks, scaled)
    _exact(site, s1, h1, ("h1",) + what)
    _exact(site, s2, h2z, ("h2 + [z|0|0]",) + what)
    _exact(site, yk, y, ("y",) + what)


_UNIT = torch.arange(384)
_MC, _MNB, _MG, _ME = _UNIT // 128, (_UNIT % 128) // 16, (_UNIT % 16) // 4, _UNIT % 4


def _gates_of(mask):
    """packed ReLU gates -> [rows, 384] bool (bit 4 nb + e of word (row, 4 c + g) <-> unit 128 c + 16 nb + 4 g + e)"""
    words = mask.cpu().long() & 0xFFFFFFFF
    return ((words[:, 4 * _MC + _MG] >> (4 * _MNB + _ME)) & 1).bool()


_GATES = {}


def _edge_gates(dev, shape, B, N, blocks):
    """gate masks from a forward whose units are all clearly positive or negative: h1 = relu(P1[i]) with P1 = +-1 (15 of 16
    positive), h2 = relu(h1[perm] - 1/2) = +-1/2; made once per launch shape and shared by the backward probes"""
    key = (dev, shape, B, N, blocks)
    if key not in _GATES:
        _GATES[key] = _edge_gates_make(dev, shape, B, N, blocks, torch.Generator().manual_seed(77 + N))
    return _GATES[key]


def _edge_gates_make(dev, shape, B, N, blocks, g):
    R, P = B * N, B * N * N
    qi, _ = _pair_index(B, N)
    P1 = torch.where(torch.rand(R, 384, generator=g) < 1.0 / 16, -1.0, 1.0)
    perm = torch.randperm(384, generator=g)
    W2 = torch.zeros(384, 384)
    W2[torch.arange(384), perm] = 1.0
    zero = lambda *s: torch.zeros(*s, device=dev)
    m1 = torch.zeros(P, 12, dtype=torch.int32, device=dev)
    m2 = torch.zeros(P, 12, dtype=torch.int32, device=dev)
    with options.override(edge_shape=shape):
        img = ops.edge_mlp_pack(zero(384, 384), W2.to(dev), zero(128, 384))
        ops.edge_mlp(zero(P, 128), img, zero(P, 128), P, N, p1=P1.to(dev), q1=zero(R, 384), bias2=torch.full((384,), -0.5, device=dev),
                     pf=zero(R, 128), qf=zero(R, 128), gamma=torch.ones(128, device=dev), beta=zero(128),
                     rowscale=torch.ones(P, device=dev), save1=zero(P, 384), save2=zero(P, 384), y=zero(P, 128), mean=zero(P),
                     rstd=zero(P), blocks=blocks, mask1=m1, mask2=m2)
    _sync(dev)
    g1 = P1[qi] > 0
    g2 = g1[:, perm]
    assert torch.equal(_gates_of(m1), g1) and torch.equal(_gates_of(m2), g2)
    return m1, m2, g1.double(), g2.double()


def _edge_bwd(dev, prod, fam, shape, B, N, blocks, seed, scaled=False):
    """backward probe of one chained product: a = (u = dy Wf), b = (d2 W2), c = (d1 W1z); A is the gradient that reaches the
    product, B the weight (sparse: 7 or 8 non-zeros per output); the other weights are signed selections"""
    g = torch.Generator().manual_seed(seed)
    ca, cb, _, nnz = FAMILIES[fam]
    P = B * N * N
    sa, sb = (2.0 ** EA, 2.0 ** EB) if scaled else (1.0, 1.0)
    m1, m2, g1, g2 = _edge_gates(dev, shape, B, N, blocks)
    dy = dense(g, ca, P, 128) * sa
    target = lambda k, n_out: sparse(g, cb, k, n_out, nnz) * sb                 # [k, n_out]: the product's B
    sel_t = lambda k, n_out, s=1.0: selection(g, n_out, k, s, neg=0.5).t().contiguous()     # [k, n_out]: one +-s per output
    W1 = dense(g, "wide", 384, 384)                                             # (columns 128..: not part of dz)
    if prod == "a":
        Wf, W2, W1z = target(128, 384), sel_t(384, 384, 1.0 / sb), torch.zeros(384, 128)
    elif prod == "b":
        Wf, W2, W1z = sel_t(128, 384), target(384, 384), sel_t(384, 128, 1.0 / sb)
    else:
        Wf, W2, W1z = sel_t(128, 384, sb), sel_t(384, 384, 1.0 / sb), target(384, 128)
    W1[:, :128] = W1z
    # ---- the exact chain and its premises
    u = dy.double() @ Wf.double()
    d2 = u * g2
    d1 = (d2 @ W2.double()) * g1
    dz = u[:, :128] + d1 @ W1z.double()
    for x in (u, d2, d1, dz):
        assert torch.equal(x.float().double(), x)
    A, Bw, add = {"a": (dy, Wf, None), "b": (d2.float(), W2, None), "c": (d1.float(), W1z, u[:, :128])}[prod]
    got = premises(A, Bw, (ca, cb), sa, sb, extra=add)
    assert torch.equal(got, {"a": u, "b": d2 @ W2.double(), "c": d1 @ W1z.double()}[prod])
    if prod == "b":
        _fits(u[:, :128].abs() + (d1 @ W1z.double()).abs(), sa, "u + d1 W1z")
    # ---- the kernel
    dev_t = lambda x: x.to(dev)
    e = lambda *s: torch.full(s, float("nan"), device=dev)
    dzk, d2k, d1k = e(P, 128), e(P, 384), e(P, 384)
    with options.override(edge_shape=shape):
        imgT = ops.edge_mlp_pack(dev_t(W1), dev_t(W2.contiguous()), dev_t(Wf.contiguous()), backward=True)
        ops.edge_mlp(dev_t(dy), imgT, dzk, P, N, gmask1=m2, gmask2=m1, save1=d2k, save2=d1k, backward=True, blocks=blocks)
    _sync(dev)
    site = f"edge_mlp_bwd_w{shape}"
    what = (prod, fam, B, N, blocks, scaled)
    _exact(site, d2k, d2, ("d2",) + what)
    _exact(site, d1k, d1, ("d1",) + what)
    _exact(site, dzk, dz, ("dz",) + what)


# (shape, B, N, blocks, scaled): 144 rows = full tiles + a ragged one; 289 rows on one block: several tiles per block
EDGE_CPU = [(4, 1, 12, 0, False), (8, 1, 17, 1, False), (4, 1, 17, 1, True), (8, 1, 12, 0, True)]
EDGE_GPU = [(4, 2, 50, 0, False), (8, 2, 50, 0, False), (4, 2, 50, 5, False), (8, 2, 50, 3, True)]


def _edge_cases(parts, cases):
    """(part, family, case); of the two scaled cases a (part, family) takes one, so that both shapes get every part scaled"""
    return [(p, f, c) for p in parts for f in (1, 2, 3) for c in cases
            if not c[4] or (f + "12fabc".index(p)) % 2 == (c[0] == 8)]


def _edge_id(v):
    return "w%d-B%d-N%d-b%d-%s" % (v[:4] + ("scaled" if v[4] else "plain",)) if isinstance(v, tuple) else str(v)


def _edge_case(dev, run, part, fam, case):
    shape, B, N, blocks, scaled = case
    run(dev, part, fam, shape, B, N, blocks, seed=400 + 100 * fam + 10 * "12fabc".index(part) + shape + N, scaled=scaled)


@pytest.mark.parametrize("layer,fam,case", _edge_cases("12f", EDGE_CPU), ids=_edge_id)
def test_edge_mlp_fwd_terms_emu(use_emu, layer, fam, case):
    _edge_case("cpu", _edge_fwd, layer, fam, case)


@pytest.mark.parametrize("prod,fam,case", _edge_cases("abc", EDGE_CPU), ids=_edge_id)
def test_edge_mlp_bwd_terms_emu(use_emu, prod, fam, case):
    _edge_case("cpu", _edge_bwd, prod, fam, case)


@pytest.mark.gpu
@pytest.mark.parametrize("layer", ["1", "2", "f"])
def test_edge_mlp_fwd_terms_gpu(hip_lib, layer):
    with _logged("edge_mlp_fwd_w4", "edge_mlp_fwd_w8"):
        for _, fam, case in _edge_cases(layer, EDGE_CPU + EDGE_GPU):
            _edge_case("cuda", _edge_fwd, layer, fam, case)


@pytest.mark.gpu
@pytest.mark.parametrize("prod", ["a", "b", "c"])
def test_edge_mlp_bwd_terms_gpu(hip_lib, prod):
    with _logged("edge_mlp_bwd_w4", "edge_mlp_bwd_w8"):
        for _, fam, case in _edge_cases(prod, EDGE_CPU + EDGE_GPU):
            _edge_case("cuda", _edge_bwd, prod, fam, case)
