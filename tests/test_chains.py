"""Chain store: training batches from backbone atoms on the device (fd_chain_windows, fd_chain_batch,
se3_diffusion_amd.data.chains.ChainStore).

Two references.  (1) np_chain: a float64 numpy restatement of include/fd_hip.h, written here; it shares nothing with the kernel.
(2) tests/golden/chain_batch.npz (tools/make_golden_chain_batch.py): the UNMODIFIED reference -- du.parse_chain_feats,
data_transforms.atom37_to_frames, atom37_to_torsion_angles, Rigid.from_tensor_4x4(rigidgroups_gt_frames)[:, 0] -- on the window
of every case, with ref_gap: per case the largest difference between the reference and the restatement on the rows where the
reference's frame exists, for rotation entries, translations and torsions.  (The reference rounds its rotations and origins to
float32 inside Rotation / Rigid; the tool prints the gaps.)

Exact against the restatement: window, lengths, res_mask, seq_idx, the identity frame of absent and padding rows, the zero
torsions and seq_idx of padding rows, the argument error of a short n_pad.

Within one fp32 ulp of float32(restatement): quaternions, torsions (2^-23: entries of magnitude <= 1) and translations
(np.spacing(float32(|value|))).  The kernel computes in fp64 and rounds once; the bound follows from that, not from a measurement.
Quaternions are compared directly: the fixture's generator asserts |w| >= 1e-6 and |C - CA|^2, |u|^2 >= 1e-3 on every present row.

Against the reference's values: rotation matrices (from the device quaternion), translations and the three torsion slots on every
row where the reference's frame exists -- all but the removed residues and the one without N: at least (L - 5) / L of a chain of
more than 16 residues.  Bound: 4 x that case's ref_gap + one fp32 ulp (2^-23 for rotation entries and torsions).

Measured, worst over the cases.  Against the restatement: 0 on the interpreter and on the device (both builds are compiled without
contraction and the restatement adds in the header's order, so the float64 values agree before the one rounding).  Against the
reference: rotation entries 8.8e-8 (6MRR), translations 0 (both sides round the same float64 value to float32), torsions 5.4e-6
on the interpreter (walk255) and 8.6e-6 on the device (walk513, which the interpreter does not run) -- the reference's own gap
on those cases, since the reference keeps its torsion frames in float32."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import parity_log  # noqa: E402
from se3_diffusion_amd import hip  # noqa: E402
from se3_diffusion_amd.data import utils as du  # noqa: E402
from se3_diffusion_amd.data.chains import ChainStore  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "chain_batch.npz")
ULP = 2.0 ** -23
EMU_MAX_LEN = 257                                  # the interpreter runs the cases up to this many residues


# ---- the float64 restatement of include/fd_hip.h ---------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _gs(p, q, r):
    """gs(p, q, r) of the header: e0 = unit(q - p), e1 = unit(v - e0 (e0 . v)) with v = r - q, e2 = e0 x e1; also the two squared
    lengths under the roots"""
    e0, v = q - p, r - q
    l0 = _dot(e0, e0)
    e0 = e0 / np.sqrt(l0 + 1e-8)[..., None]
    e1 = v - e0 * _dot(e0, v)[..., None]
    l1 = _dot(e1, e1)
    e1 = e1 / np.sqrt(l1 + 1e-8)[..., None]
    e2 = np.stack([e0[..., 1] * e1[..., 2] - e0[..., 2] * e1[..., 1], e0[..., 2] * e1[..., 0] - e0[..., 0] * e1[..., 2],
                   e0[..., 0] * e1[..., 1] - e0[..., 1] * e1[..., 0]], -1)
    return e0, e1, e2, l0, l1


def _torsion(a, b, c, d):
    _, e1, e2, _, _ = _gs(b, c, a)
    w = d - c
    ry, rz = _dot(e1, w), _dot(e2, w)
    den = np.sqrt((rz * rz + ry * ry) + 1e-8)
    return np.stack([rz / den, ry / den], -1)


def np_window(mask):
    present = (np.asarray(mask)[:, :3] != 0).all(-1) if len(mask) else np.zeros(0, bool)
    k = np.flatnonzero(present)
    return (int(k[0]), int(k[-1]), len(k)) if len(k) else (0, -1, 0)


def np_chain(atoms, mask, res_index, n_pad=None):
    """one entry of fd_chain_batch: atoms float32 [L,4,3], mask [L,4], res_index [L] -> dict of float64 / integer arrays over n_pad
    rows (None: the window), the rotation matrices of the window rows, and the decision margins of the present rows"""
    first, last, count = np_window(mask)
    W = last - first + 1
    n_pad = W if n_pad is None else n_pad
    assert n_pad >= W
    on = np.asarray(mask)[first:last + 1] != 0
    raw = np.asarray(atoms)[first:last + 1].astype(np.float64)
    # centre: thread t of 256 adds rows t, t + 256, ..; butterfly within each wave of 64; (s0 + s1) + (s2 + s3)
    part = np.zeros((256, 3))
    for k in range(0, W, 256):
        rows = slice(k, min(k + 256, W))
        part[:rows.stop - k] += np.where(on[rows, 1, None], raw[rows, 1], 0.0)
    part = part.reshape(4, 64, 3)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[:, np.arange(64) ^ o]
    ctr = ((part[0, 0] + part[1, 0]) + (part[2, 0] + part[3, 0])) / (float(on[:, 1].sum()) + 1e-5)
    x = np.where(on[..., None], raw - ctr, 0.0)                  # [W,4,3]: N, CA, C, O, centred, absent atoms at the origin
    prev = np.concatenate([np.zeros((1, 4, 3)), x[:-1]]) if W else x
    N, CA, C, O = x[:, 0], x[:, 1], x[:, 2], x[:, 3]
    tors = np.zeros((n_pad, 7, 2))
    rig = np.zeros((n_pad, 7))
    rig[:, 0] = 1.0
    res_mask, seq_idx = np.zeros(n_pad), np.zeros(n_pad, np.int64)
    rot = np.zeros((W, 3, 3))
    margin = dict(w=np.inf, l0=np.inf, l1=np.inf)
    if W:
        tors[:W, 0] = _torsion(prev[:, 1], prev[:, 2], N, CA)
        tors[:W, 1] = _torsion(prev[:, 2], N, CA, C)
        tors[:W, 2] = -_torsion(N, CA, C, O)
        present = on[:, :3].all(-1)
        ex, ey, ez, l0, l1 = _gs(CA, C, N)
        R = np.stack([ex, ey, ez], -1)                           # columns x, y, z
        t = np.stack([((1.0 + R[:, 0, 0]) + R[:, 1, 1]) + R[:, 2, 2], ((1.0 + R[:, 0, 0]) - R[:, 1, 1]) - R[:, 2, 2],
                      ((1.0 - R[:, 0, 0]) + R[:, 1, 1]) - R[:, 2, 2], ((1.0 - R[:, 0, 0]) - R[:, 1, 1]) + R[:, 2, 2]], -1)
        a, b, c = R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]
        d, e, f = R[:, 0, 1] + R[:, 1, 0], R[:, 0, 2] + R[:, 2, 0], R[:, 1, 2] + R[:, 2, 1]
        cand = np.stack([np.stack([t[:, 0], a, b, c], -1), np.stack([a, t[:, 1], d, e], -1), np.stack([b, d, t[:, 2], f], -1),
                         np.stack([c, e, f, t[:, 3]], -1)], 1)   # [W, branch, 4]
        q = cand[np.arange(W), np.argmax(t, -1)]                 # (argmax: the first on ties)
        nq = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
        q = q / np.where(q[:, 0] < 0, -nq, nq)[:, None]
        rig[:W][present] = np.concatenate([q, CA], -1)[present]
        res_mask[:W] = present
        idx = np.asarray(res_index)[first:last + 1].astype(np.int64)
        seq_idx[:W] = idx - idx.min() + 1
        rot = R
        if present.any():
            margin = dict(w=float(np.abs(q[present, 0]).min()), l0=float(l0[present].min()), l1=float(l1[present].min()))
    return dict(window=(first, last, count), rigids_0=rig, torsions=tors, res_mask=res_mask, seq_idx=seq_idx, rot=rot, margin=margin)


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gold():
    return np.load(GOLD)


def _names():
    return tuple(str(x) for x in _gold()["names"])


@functools.lru_cache(maxsize=None)
def _case(name):
    """inputs (atoms [L,4,3], mask [L,4], res_index [L]), the restatement (n_pad = window + 3), the reference's values on the window
    and ref_gap = (rotation, translation, torsion); computed once, shared by both tiers, never modified"""
    G = _gold()
    k = _names().index(name)
    rows = slice(int(G["row_start"][k]), int(G["row_start"][k + 1]))
    win = slice(int(G["win_start"][k]), int(G["win_start"][k + 1]))
    inp = (G["atoms"][rows], G["mask"][rows], G["res_index"][rows])
    first, last, _ = np_window(inp[1])
    ref = np_chain(*inp, n_pad=last - first + 1 + 3)
    gold = dict(rot=G["ref_rot"][win].astype(np.float64), trans=G["ref_trans"][win].astype(np.float64),
                exists=G["ref_exists"][win] != 0, tors=G["ref_tors"][win].astype(np.float64))
    assert len(gold["rot"]) == last - first + 1
    return inp, ref, gold, tuple(float(g) for g in G["ref_gap"][k])


def _t(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dev)


def _store(dev, chains):
    s = ChainStore(dev)
    for atoms, mask, idx in chains:
        s.add(atoms=atoms, atom_mask=mask, residue_index=idx)
    return s.freeze()


def _np(x):
    return x.detach().cpu().numpy()


def _check_restated(tag, got, ref, row_lo=0):
    """one entry (dict of numpy arrays [n_pad, ...]) against the restatement"""
    n_pad = len(ref["res_mask"])
    W = ref["window"][1] - ref["window"][0] + 1
    assert got["res_mask"].dtype == np.float32 and np.array_equal(got["res_mask"], ref["res_mask"]), tag
    assert got["seq_idx"].dtype == np.int64 and np.array_equal(got["seq_idx"], ref["seq_idx"]), tag
    off = ref["res_mask"] == 0
    ident = np.array([1, 0, 0, 0, 0, 0, 0], np.float32)
    assert (got["rigids_0"][off] == ident).all(), (tag, "absent and padding rows carry the identity frame")
    assert not got["torsion_angles_sin_cos"][W:].any() and not got["seq_idx"][W:].any(), (tag, "padding rows are zero")
    assert not got["torsion_angles_sin_cos"][:, 3:].any(), (tag, "slots 3..6")
    r32 = ref["rigids_0"].astype(np.float32)
    eq = float(np.abs(got["rigids_0"][:, :4].astype(np.float64) - r32[:, :4]).max()) if n_pad else 0.0
    et = float(np.abs(got["torsion_angles_sin_cos"].astype(np.float64) - ref["torsions"].astype(np.float32)).max()) if n_pad else 0.0
    dx = np.abs(got["rigids_0"][:, 4:].astype(np.float64) - r32[:, 4:])
    ex = float((dx / np.spacing(np.abs(r32[:, 4:]))).max()) if n_pad else 0.0       # in ulps of the value
    for key, e in (("quat", eq), ("torsion", et)):
        parity_log.out(f"{tag}.restated.{key}", e)
        print(f"  {tag}.restated.{key}: achieved {e:.3e} (bound {ULP:.2e})")
        assert e <= ULP, (tag, key, e)
    parity_log.out(f"{tag}.restated.trans_ulps", ex)
    print(f"  {tag}.restated.trans: achieved {ex:.2f} ulp (bound 1)")
    assert ex <= 1.0, (tag, ex)


def _entry(out, p):
    return {k: _np(v[p]) for k, v in out.items()}


# ---- 1. the cases of the fixture ------------------------------------------------------------------------------------------------------
def _run_case(dev, name):
    with parity_log.case(f"chains_{name}[{dev}]"):
        (atoms, mask, idx), ref, gold, gap = _case(name)
        first, last, count = ref["window"]
        W = last - first + 1
        store = _store(dev, [(atoms, mask, idx)])
        assert store.windows.dtype == np.int32 and store.windows.tolist() == [[first, last, count]], (name, store.windows)
        assert store.lengths.tolist() == [W]
        out = store.build_batch([0], n_pad=W + 3)
        assert out["rigids_0"].shape == (1, W + 3, 7) and out["torsion_angles_sin_cos"].shape == (1, W + 3, 7, 2)
        assert out["gt_bb"].shape == (1, W + 3, 5, 3)
        got = _entry(out, 0)
        print(f"  {name}: L {len(atoms)} window {first}..{last} present {count} margin {ref['margin']}")
        _check_restated(name, got, ref)
        assert int(got["res_mask"].sum()) == count
        if W == 0:
            return
        # the reference's values, on the rows where its frame exists
        ex = gold["exists"]
        assert np.array_equal(ex, ref["res_mask"][:W] != 0), (name, "the reference's frame exists where N, CA and C are present")
        if W > 16:
            assert ex.sum() >= W - 5, (name, ex.sum(), W)
        rot = du.quat_wxyz_to_matrix(got["rigids_0"][:W, :4].astype(np.float64))
        e_rot = float(np.abs(rot - gold["rot"])[ex].max())
        dx = np.abs(got["rigids_0"][:W, 4:].astype(np.float64) - gold["trans"])[ex]
        ulp_x = np.spacing(np.abs(got["rigids_0"][:W, 4:]))[ex].astype(np.float64)
        e_trans, ok_trans = float(dx.max()), bool((dx <= 4 * gap[1] + ulp_x).all())
        e_tor = float(np.abs(got["torsion_angles_sin_cos"][:W, :3].astype(np.float64) - gold["tors"])[ex].max())
        for key, e, bound in (("rot", e_rot, 4 * gap[0] + ULP), ("trans", e_trans, 4 * gap[1]), ("torsion", e_tor, 4 * gap[2] + ULP)):
            parity_log.out(f"{name}.ref.{key}", e)
            print(f"  {name}.ref.{key}: achieved {e:.3e} (bound {bound:.2e}{' + one ulp of the value' if key == 'trans' else ''})")
        assert e_rot <= 4 * gap[0] + ULP and ok_trans and e_tor <= 4 * gap[2] + ULP, (name, e_rot, e_trans, e_tor, gap)


def _emu_names():
    G = _gold()
    return [n for k, n in enumerate(_names()) if int(G["row_start"][k + 1] - G["row_start"][k]) <= EMU_MAX_LEN]


def pytest_generate_tests(metafunc):
    if "emu_case" in metafunc.fixturenames:
        metafunc.parametrize("emu_case", _emu_names())
    if "gpu_case" in metafunc.fixturenames:
        metafunc.parametrize("gpu_case", _names())


def test_case_emu(use_emu, emu_case):
    _run_case("cpu", emu_case)


@pytest.mark.gpu
def test_case_gpu(hip_lib, gpu_case):
    _run_case("cuda", gpu_case)


def test_fixture_is_what_the_issue_asks():
    """the cases and the decision margins the comparisons rest on"""
    G = _gold()
    names = _names()
    lens = {n: int(G["row_start"][k + 1] - G["row_start"][k]) for k, n in enumerate(names)}
    for pdb in ("4GYT", "4YOW", "6MRR", "3HTN", "5L33", "6EHB"):
        assert pdb in names
    assert {1, 2, 63, 64, 65, 255, 256, 257, 513} <= {lens[n] for n in names if n.startswith("walk")}
    assert os.path.getsize(GOLD) < 1_000_000
    for n in names:
        (atoms, mask, idx), ref, gold, gap = _case(n)
        first, last, count = ref["window"]
        W = last - first + 1
        if count:
            assert ref["margin"]["w"] >= 1e-6 and ref["margin"]["l0"] >= 1e-3 and ref["margin"]["l1"] >= 1e-3, (n, ref["margin"])
        if lens[n] > 16:                                         # the modifications
            on = mask != 0
            assert first > 0 and last < lens[n] - 1, (n, "absent residues at both ends")
            inner = on[first:last + 1]
            assert (~inner.any(-1)).sum() == 3, (n, "three whole residues removed")
            assert ((inner[:, :3].all(-1)) & ~inner[:, 3]).sum() == 1, (n, "one residue without O")
            assert (~inner[:, 0] & inner[:, 1:].all(-1)).sum() == 1, (n, "one residue without N")
            assert count == W - 4
    assert _case("single")[1]["window"][2] == 1 and _case("empty")[1]["window"] == (0, -1, 0)


# ---- 2. bits: alone, elsewhere in a batch, padded, behind another chain, repeated, garbage where nothing is read -----------------------
def _walk(rng, n):
    """a random chain: CA walk of 3.8 A steps, N, C and O at bond lengths in random directions"""
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    ca = np.cumsum(3.8 * unit(rng.normal(size=(n, 3))), 0) + rng.normal(size=3) * 20
    nn, c = ca + 1.46 * unit(rng.normal(size=(n, 3))), ca + 1.52 * unit(rng.normal(size=(n, 3)))
    o = c + 1.23 * unit(rng.normal(size=(n, 3)))
    return np.stack([nn, ca, c, o], 1).astype(np.float32)


def _chains3():
    rng = np.random.default_rng(7)
    a = (_walk(rng, 70), np.ones((70, 4), np.uint8), np.arange(70) + 5)
    b = (_walk(rng, 300), np.ones((300, 4), np.uint8), np.arange(300) * 2 - 40)
    c = (_walk(rng, 41), np.ones((41, 4), np.uint8), np.arange(41))
    b[1][[0, 1, 298, 299]] = 0                                   # trimmed at both ends: window 2..297
    b[1][100] = 0
    b[1][200, 0] = 0
    b[1][3, 3] = 0
    c[1][40, 2] = 0                                              # its last residue has CA but no C: outside the window
    return a, b, c


def _same(x, y, rows=None):
    return all(torch.equal(x[k][:rows] if rows else x[k], y[k][:rows] if rows else y[k]) for k in x)


def _run_bits(dev):
    a, b, c = _chains3()
    store = _store(dev, [a, b, c])
    assert store.lengths.tolist() == [70, 296, 40]
    ref = np_chain(*b)
    Wb = 296
    alone = store.build_batch([1])
    _check_restated("bits.b", _entry(alone, 0), ref)
    one = {k: v[0] for k, v in alone.items()}
    three = store.build_batch([1, 0, 2])                         # as entry 0 of 3
    assert _same(one, {k: v[0] for k, v in three.items()})
    three = store.build_batch([2, 0, 1], n_pad=Wb + 7)           # as entry 2 of 3, with seven rows of padding
    assert _same(one, {k: v[2] for k, v in three.items()}, rows=Wb)
    pad = _entry(three, 2)
    assert not pad["res_mask"][Wb:].any() and not pad["seq_idx"][Wb:].any() and not pad["torsion_angles_sin_cos"][Wb:].any()
    assert (pad["rigids_0"][Wb:] == np.array([1, 0, 0, 0, 0, 0, 0], np.float32)).all()
    _check_restated("bits.c", _entry(three, 0), np_chain(*c, n_pad=Wb + 7))
    # another chain in front of it in the store
    other = _store(dev, [c, c, b])
    assert _same(one, {k: v[0] for k, v in other.build_batch([2]).items()})
    # repeated ids: identical rows
    rep = store.build_batch([1, 1, 0, 1])
    for p in (1, 3):
        assert _same({k: v[0] for k, v in rep.items()}, {k: v[p] for k, v in rep.items()})
    # the coordinates of absent atoms and the residues outside the window are never read into a result
    atoms, mask, idx = b[0].copy(), b[1], b[2].copy()
    atoms[mask == 0] = np.nan
    atoms[[0, 299]] = 3.0e30
    idx[[0, 1, 298, 299]] = -(2 ** 30)
    dirty = _store(dev, [(atoms, mask, idx)])
    assert _same(one, {k: v[0] for k, v in dirty.build_batch([0]).items()})


def test_bits_emu(use_emu):
    _run_bits("cpu")


@pytest.mark.gpu
def test_bits_gpu(hip_lib):
    _run_bits("cuda")


# ---- 3. the refused arguments ------------------------------------------------------------------------------------------------------------
def _run_arguments(dev, lib):
    a, b, c = _chains3()
    store = _store(dev, [a, c])
    n0 = lib.cdll.fd_launch_count()
    with pytest.raises(ValueError, match="shorter than a window of 70"):
        store.build_batch([1, 0], n_pad=69)
    with pytest.raises(ValueError, match="chain ids"):
        store.build_batch([2])
    with pytest.raises(ValueError, match="chain ids"):
        store.build_batch([-1])
    with pytest.raises(RuntimeError, match="freeze"):
        ChainStore(dev).build_batch([0])
    with pytest.raises(RuntimeError, match="freeze"):
        store.add(atoms=a[0], atom_mask=a[1], residue_index=a[2])
    with pytest.raises(ValueError, match="expected atoms"):
        ChainStore(dev).add(atoms=np.zeros((5, 3, 3)), atom_mask=np.zeros((5, 3)))
    f = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)
    ids = f(1, dt=torch.int32)
    from se3_diffusion_amd import trunk
    outs = (f(1, 70, 7), f(1, 70, 7, 2), f(1, 70), f(1, 70, dt=torch.int64))
    with pytest.raises(hip.FdError, match="null output"):
        lib.call("fd_chain_batch", store.atoms, store.atom_mask, store.res_index, store.offsets, store._window, ids, 1, 70,
                 trunk.head_const(), None, *outs[1:], None)
    with pytest.raises(hip.FdError, match="null store operand"):
        lib.call("fd_chain_batch", store.atoms, store.atom_mask, None, store.offsets, store._window, ids, 1, 70,
                 trunk.head_const(), *outs, None)
    with pytest.raises(hip.FdError, match="negative"):
        lib.call("fd_chain_batch", store.atoms, store.atom_mask, store.res_index, store.offsets, store._window, ids, 1, -1,
                 trunk.head_const(), *outs, None)
    with pytest.raises(hip.FdError, match="null"):
        lib.call("fd_chain_windows", store.atoms, None, store.offsets, 2, store._window)
    assert lib.cdll.fd_launch_count() == n0                      # refused: nothing was launched
    # a store without chains, a batch without entries: nothing is launched
    empty = ChainStore(dev).freeze()
    assert empty.lengths.shape == (0,) and empty.build_batch([])["rigids_0"].shape == (0, 0, 7)
    assert store.build_batch([], n_pad=4)["seq_idx"].shape == (0, 4)
    assert lib.cdll.fd_launch_count() == n0
    # the reference's dict: atom37 columns 0, 1, 2, 4
    pos, msk = np.zeros((70, 37, 3), np.float32), np.zeros((70, 37), np.float32)
    pos[:, [0, 1, 2, 4]], msk[:, [0, 1, 2, 4]] = a[0], 1
    pos[:, 3], msk[:, 3] = 7.0, 1                                # CB is not taken
    s37 = ChainStore(dev)
    s37.add({"atom_positions": pos, "atom_mask": msk, "residue_index": a[2]})
    assert _same(store.build_batch([0]), s37.freeze().build_batch([0]))


def test_arguments_emu(use_emu):
    _run_arguments("cpu", use_emu)


@pytest.mark.gpu
def test_arguments_gpu(hip_lib):
    _run_arguments("cuda", hip_lib)


# ---- 4. composition with the existing noising and the existing backbone builder -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _diffuser():
    from se3_diffusion_amd.data import se3_diffuser
    from test_diffuser import conf as dconf
    return se3_diffuser.SE3Diffuser(dconf())


def _step_chains():
    """windows of 17, 24 and 24 residues with 16, 24 and 23 present ones"""
    rng = np.random.default_rng(11)
    a = (_walk(rng, 19), np.ones((19, 4), np.uint8), np.arange(19) + 3)
    b = (_walk(rng, 24), np.ones((24, 4), np.uint8), np.arange(24))
    c = (_walk(rng, 24), np.ones((24, 4), np.uint8), np.arange(24) + 100)
    a[1][[0, 18, 9]] = 0
    c[1][5, 0] = 0
    return a, b, c


def _run_composition(dev):
    from se3_diffusion_amd import train_step as ts
    diff = _diffuser()
    store = _store(dev, _step_chains())
    assert store.lengths.tolist() == [17, 24, 24]
    B, N = 3, 24
    rs = np.random.RandomState(3)
    noise = (rs.standard_normal((B, N, 3)), rs.uniform(size=(B, N)), rs.standard_normal((B, N, 3)))
    t = np.array([0.21, 0.5, 0.93])
    batch, gt = store.training_batch([0, 1, 2], diff, t=t, noise=noise)
    want = ts.synthetic_batch(B, N, dev)
    assert list(batch) == list(want)
    for k in want:
        assert batch[k].dtype == want[k].dtype and batch[k].shape == want[k].shape and batch[k].device == want[k].device, k
    assert not batch["fixed_mask"].any() and not batch["sc_ca_t"].any()
    assert torch.equal(batch["t"], torch.tensor(t, dtype=torch.float32, device=dev))
    assert batch["res_mask"].sum(1).tolist() == [16.0, 24.0, 23.0]
    direct = diff.forward_marginal_batch(batch["rigids_0"], t, diffuse_mask=batch["res_mask"], noise=noise)
    for k in ("rigids_t", "rot_score", "trans_score", "rot_score_scaling", "trans_score_scaling"):
        assert torch.equal(batch[k], direct[k]), k
    off = batch["res_mask"] == 0                                 # the noising kernel copies the frame and writes zero scores
    assert torch.equal(batch["rigids_t"][off], batch["rigids_0"][off]) and not batch["rot_score"][off].any()
    assert gt.shape == (B, N, 37, 3) and gt.dtype == torch.float32 and not gt[:, :, 5:].any()
    a37, _ = ts.backbone_atoms(batch["rigids_0"], batch["torsion_angles_sin_cos"][..., 2, :])
    assert torch.equal(gt[..., :5, :], a37[..., :5, :])
    # t by default: rng.uniform(min_t, 1) per entry; the same chain at different times is the reference's time_batch
    tb, _ = store.training_batch([1, 1, 1], diff, rng=np.random.default_rng(5), noise=noise)
    assert torch.equal(tb["t"], torch.tensor(np.random.default_rng(5).uniform(0.01, 1.0, size=3), dtype=torch.float32, device=dev))
    assert torch.equal(tb["rigids_0"][0], tb["rigids_0"][2]) and not torch.equal(tb["rigids_t"][0], tb["rigids_t"][2])


def test_composition_emu(use_emu):
    _run_composition("cpu")


@pytest.mark.gpu
def test_composition_gpu(hip_lib):
    _run_composition("cuda")


# ---- 5. one training step on a built batch -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_training_step_gpu(hip_lib):
    from se3_diffusion_amd import loss as floss, train_step as ts
    from se3_diffusion_amd.model.score_network import ScoreNetwork
    dev = "cuda"
    diff = _diffuser()
    store = _store(dev, _step_chains())
    gen = torch.Generator(device=dev).manual_seed(2)
    batch, gt = store.training_batch([0, 1, 2], diff, t=np.array([0.1, 0.2, 0.9]), generator=gen)
    assert batch["res_mask"].shape == (3, 24)
    torch.manual_seed(0)
    model = ScoreNetwork(ts.base_model_conf(num_blocks=1), diff).to(dev)
    ts.perturb_final_layers(model, seed=0)
    model.train()
    out = model(batch)
    loss, terms = floss.dsm_loss(batch, out, gt, with_terms=True)
    loss.backward()
    assert torch.isfinite(loss).all()
    for k in ("rot_score", "trans_score", "rigids", "atom37", "psi"):
        assert torch.isfinite(out[k]).all(), k
    for k, v in terms.items():
        assert torch.isfinite(v).all(), k
    grads = [(n, p.grad) for n, p in model.named_parameters() if p.requires_grad]
    assert all(g is not None and torch.isfinite(g).all() for _, g in grads), [n for n, g in grads if g is None or not torch.isfinite(g).all()]
    assert any(float(g.abs().max()) > 0 for _, g in grads)
    assert terms["loss_mask_sum"].tolist() == [16.0, 24.0, 23.0]


# ---- 6. batches(..): the reference's length_batch mode ----------------------------------------------------------------------------------
def _run_batches(dev):
    diff = _diffuser()
    rng = np.random.default_rng(23)
    lens = [5, 7, 5, 9, 7, 5, 0, 5, 7, 9, 5, 12]
    chains = []
    for n in lens:
        m = np.ones((n + 2, 4), np.uint8)
        m[[0, -1]] = 0                                           # the window is n residues; n = 0: no present residue at all
        if n == 0:
            m[:] = 0
        chains.append((_walk(rng, n + 2), m, np.arange(n + 2)))
    store = _store(dev, chains)
    assert store.lengths.tolist() == lens
    batch_size, msr = 2, 2 * 49 + 10                             # N = 5, 7: two per batch; N = 9: one; N = 12: none fits

    def run(seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        return list(store.batches(batch_size, msr, np.random.default_rng(seed), diff, generator=g))

    first, again, other = run(1), run(1), run(2)
    plan = store.batch_plan(batch_size, msr, np.random.default_rng(1))
    assert len(first) == len(plan) == 3 + 2 + 2
    seen = np.concatenate(plan)
    assert sorted(seen.tolist()) == [k for k, n in enumerate(lens) if n in (5, 7, 9)]          # each once; 0 and 12 are left out
    for ids, batch in zip(plan, first):
        B, N = batch["res_mask"].shape
        assert len(set(store.lengths[ids].tolist())) == 1 and N == store.lengths[ids[0]] and B == len(ids)
        assert B * N * N <= msr and B <= batch_size
        assert batch["res_mask"].all() and batch["seq_idx"][:, 0].eq(1).all()
        assert torch.equal(batch["rigids_0"], store.build_batch(ids)["rigids_0"])
        assert batch["rigids_0"].device.type == torch.device(dev).type
    for x, y in zip(first, again):                               # a fixed rng (and generator): a fixed sequence
        assert all(torch.equal(x[k], y[k]) for k in x)
    assert [b["res_mask"].shape for b in first] != [b["res_mask"].shape for b in other] or \
        not all(torch.equal(x["t"], y["t"]) for x, y in zip(first, other))
    pairs = list(store.batches(batch_size, msr, np.random.default_rng(1), diff, with_gt=True))
    assert all(gt.shape == b["res_mask"].shape + (37, 3) for b, gt in pairs)


def test_batches_emu(use_emu):
    _run_batches("cpu")


@pytest.mark.gpu
def test_batches_gpu(hip_lib):
    _run_batches("cuda")
