"""Kernel-level parity: every HIP entry point of the C-ABI against the CPU oracle on the
same seeded inputs.  Field stencils, filter and guard-cell kernels keep the reference's
operation order and must be bit-identical; per-particle kernels may differ by FMA
contraction (tolerance 1e-12 of the field scale); deposition sums in a different order
(atomics) and is compared per cell at 1e-12 of max|J|."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import helpers as H
from warpx_amd import _capi, plasma
from warpx_amd.containers import STAG, FieldArray, ParticleArrays, field_triplet

pytestmark = pytest.mark.gpu

DEV = H.DEVICE
NCELL = (24, 20, 16)


def _sync(product):
    product.device_synchronize()


@pytest.mark.parametrize("pad", [False, True])
def test_evolve_b_bit_exact(oracle, product, pad):
    ng = 2
    E = H.random_fields(("Ex", "Ey", "Ez"), NCELL, ng, 1)
    B = H.random_fields(("Bx", "By", "Bz"), NCELL, ng, 2)
    Ed, Bd = H.clone_fields(E, DEV, pad), H.clone_fields(B, DEV, pad)
    _, dx = H.geom_for(NCELL, ng)
    dt = 0.5 * H.yee_dt(dx)
    dinv = H.d3(1.0 / dx)
    oracle.evolve_b(field_triplet(E), field_triplet(B), dt, dinv, None)
    product.evolve_b(field_triplet(Ed), field_triplet(Bd), dt, dinv, None)
    _sync(product)
    for a, b in zip(Bd, B):
        assert np.array_equal(a.to_numpy(), b.to_numpy())


@pytest.mark.parametrize("pad", [False, True])
def test_evolve_e_bit_exact(oracle, product, pad):
    ng = 2
    E = H.random_fields(("Ex", "Ey", "Ez"), NCELL, ng, 3)
    B = H.random_fields(("Bx", "By", "Bz"), NCELL, ng, 4, scale=1e-8)
    J = H.random_fields(("jx", "jy", "jz"), NCELL, 3, 5, scale=1e3)
    Ed, Bd, Jd = (H.clone_fields(x, DEV, pad) for x in (E, B, J))
    _, dx = H.geom_for(NCELL, ng)
    dt = H.yee_dt(dx)
    dinv = H.d3(1.0 / dx)
    oracle.evolve_e(field_triplet(E), field_triplet(B), field_triplet(J), dt, dinv, None)
    product.evolve_e(field_triplet(Ed), field_triplet(Bd), field_triplet(Jd), dt, dinv, None)
    _sync(product)
    for a, b in zip(Ed, E):
        assert np.array_equal(a.to_numpy(), b.to_numpy())


def test_evolve_unsupported_staggering(product):
    f = [FieldArray(NCELL, (1, 1, 1), (2, 2, 2), DEV) for _ in range(6)]
    with pytest.raises(_capi.WxaError):
        product.evolve_b(field_triplet(f[:3]), field_triplet(f[3:]), 1e-16, H.d3((1, 1, 1)), None)


@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("galerkin", [1, 0])
@pytest.mark.parametrize("pusher", [_capi.PUSHER_BORIS, _capi.PUSHER_VAY])
def test_gather_push(oracle, product, order, galerkin, pusher):
    ng, _, _ = H.guard_depths(order)
    E = H.random_fields(("Ex", "Ey", "Ez"), NCELL, ng, 10, scale=1e11)
    B = H.random_fields(("Bx", "By", "Bz"), NCELL, ng, 11, scale=1e3)
    Ed, Bd = H.clone_fields(E, DEV, True), H.clone_fields(B, DEV, True)
    parts = H.random_particles(5000, NCELL, 12)
    ph = ParticleArrays.from_numpy(parts, "cpu")
    pd = ParticleArrays.from_numpy(parts, DEV)
    g, dx = H.geom_for(NCELL, ng)
    dt = H.yee_dt(dx)
    q, m = -plasma.Q_E, plasma.M_E
    for fn in ("gather_push", "push_p"):
        getattr(oracle, fn)(C.byref(ph.view), field_triplet(E), field_triplet(B), C.byref(g), q, m, dt,
                            order, galerkin, pusher, None)
        getattr(product, fn)(C.byref(pd.view), field_triplet(Ed), field_triplet(Bd), C.byref(g), q, m, dt,
                             order, galerkin, pusher, None)
        _sync(product)
        a, b = pd.to_numpy(), ph.to_numpy()
        for row in range(7):
            assert H.max_rel_err(a[row], b[row]) < 1e-12, (fn, row)


@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("algo", [_capi.DEPOSIT_ESIRKEPOV, _capi.DEPOSIT_DIRECT])
def test_deposit_current(oracle, product, order, algo):
    _, ng_depos, ng_j = H.guard_depths(order, use_filter=True)
    J = [FieldArray(NCELL, STAG[n], (ng_j,) * 3, "cpu") for n in ("jx", "jy", "jz")]
    Jd = H.clone_fields(J, DEV, True)
    parts = H.random_particles(20000, NCELL, 20 + order, u_scale=1.0)
    ph = ParticleArrays.from_numpy(parts, "cpu")
    pd = ParticleArrays.from_numpy(parts, DEV)
    g, dx = H.geom_for(NCELL, ng_depos)
    dt = H.yee_dt(dx)
    q = -plasma.Q_E
    oracle.deposit_current(C.byref(ph.view), field_triplet(J), C.byref(g), q, dt, -0.5 * dt, order, algo, None, None)
    product.deposit_current(C.byref(pd.view), field_triplet(Jd), C.byref(g), q, dt, -0.5 * dt, order, algo, None, None)
    _sync(product)
    for a, b in zip(Jd, J):
        assert H.max_rel_err(a.to_numpy(), b.to_numpy()) < 1e-12
    # empty input is a no-op
    empty = ParticleArrays(0, DEV)
    product.deposit_current(C.byref(empty.view), field_triplet(Jd), C.byref(g), q, dt, -0.5 * dt, order, algo, None, None)


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_esirkepov_continuity(product, order):
    """Discrete continuity (rho_new - rho_old)/dt + div J = 0 to round-off (Esirkepov 2001):
    an analytic property of the path that no reference test pins."""
    resid = H.continuity_residual(product, DEV, order, NCELL)
    assert resid < 1e-11


@pytest.mark.parametrize("order", [1, 3, 4])
def test_deposit_charge(oracle, product, order):
    ng = order + 2
    rho = FieldArray(NCELL, STAG["rho"], (ng,) * 3, "cpu")
    rhod = rho.copy_to(DEV, True)
    parts = H.random_particles(8000, NCELL, 40)
    ph, pd = ParticleArrays.from_numpy(parts, "cpu"), ParticleArrays.from_numpy(parts, DEV)
    g, _ = H.geom_for(NCELL, ng)
    oracle.deposit_charge(C.byref(ph.view), C.byref(rho.view), C.byref(g), plasma.Q_E, order, None)
    product.deposit_charge(C.byref(pd.view), C.byref(rhod.view), C.byref(g), plasma.Q_E, order, None)
    _sync(product)
    assert H.max_rel_err(rhod.to_numpy(), rho.to_numpy()) < 1e-12


def test_filter_bit_exact(oracle, product):
    (src,) = H.random_fields(("jx",), NCELL, 4, 50)
    dst = src.like()
    srcd, dstd = src.copy_to(DEV, True), src.like(DEV, True)
    oracle.filter_bilinear(C.byref(src.view), C.byref(dst.view), None)
    product.filter_bilinear(C.byref(srcd.view), C.byref(dstd.view), None)
    _sync(product)
    assert np.array_equal(dstd.to_numpy(), dst.to_numpy())
    with pytest.raises(_capi.WxaError):
        product.filter_bilinear(C.byref(srcd.view), C.byref(srcd.view), None)


@pytest.mark.parametrize("name,lens", [("Ex", (1, 1, 5)), ("Bz", (1, 1, 5)), ("Ey", (2, 2, 2)), ("Bx", (3, 1, 4))])
@pytest.mark.parametrize("ncell", [(20, 12, 28), (9, 5, 131)])
def test_filter_stencil_bit_exact(oracle, product, name, lens, ncell):
    """wxa_filter_stencil (Filter::DoFilter with any half stencils): the NCI corrector's 1 x 1 x 5 Godfrey stencil from
    wxa_nci_godfrey_stencil, the bilinear filter's 2 x 2 x 2 through the generic kernel, and an odd mix -- bit for bit
    against the CPU restatement (same loop and term order, no contraction)."""
    (src,) = H.random_fields((name,), ncell, 4, 51)   # (131 + guards along z: five segments of the 1 x 1 x 5 kernel's march)
    dst = src.like()
    srcd, dstd = src.copy_to(DEV, True), src.like(DEV, True)
    rng = np.random.default_rng(3)
    st = []
    for d in range(3):
        if lens == (1, 1, 5) and d == 2:
            z = (C.c_double * 5)()
            product.nci_godfrey_stencil(0.577, 0, 0 if name == "Ex" else 1, z)
            zo = (C.c_double * 5)()
            oracle.nci_godfrey_stencil(0.577, 0, 0 if name == "Ex" else 1, zo)
            assert list(z) == list(zo)
            st.append(z)
        elif lens[d] == 1:
            st.append((C.c_double * 1)(0.5))
        else:
            st.append((C.c_double * lens[d])(*rng.random(lens[d])))
    oracle.filter_stencil(C.byref(src.view), C.byref(dst.view), st[0], lens[0], st[1], lens[1], st[2], lens[2], None)
    product.filter_stencil(C.byref(srcd.view), C.byref(dstd.view), st[0], lens[0], st[1], lens[1], st[2], lens[2], None)
    _sync(product)
    assert np.array_equal(dstd.to_numpy(), dst.to_numpy())
    with pytest.raises(_capi.WxaError):
        product.filter_stencil(C.byref(srcd.view), C.byref(srcd.view), st[0], lens[0], st[1], lens[1], st[2], lens[2], None)


@pytest.mark.parametrize("name", ["Ex", "By", "rho"])
@pytest.mark.parametrize("ng_fill", [1, 2, 4])
def test_fill_boundary_bit_exact(oracle, product, name, ng_fill):
    (f,) = H.random_fields((name,), NCELL, 4, 60)
    fd = f.copy_to(DEV, True)
    per = H.i3((1, 1, 1))
    oracle.sync_nodal_periodic(C.byref(f.view), per, None)
    oracle.fill_boundary_periodic(C.byref(f.view), H.i3((ng_fill,) * 3), per, None)
    product.sync_nodal_periodic(C.byref(fd.view), per, None)
    product.fill_boundary_periodic(C.byref(fd.view), H.i3((ng_fill,) * 3), per, None)
    _sync(product)
    assert np.array_equal(fd.to_numpy(), f.to_numpy())


@pytest.mark.parametrize("name", ["jx", "jz", "rho"])
@pytest.mark.parametrize("src_ng", [2, 4])
def test_sum_boundary(oracle, product, name, src_ng):
    (f,) = H.random_fields((name,), NCELL, 4, 70)
    fd = f.copy_to(DEV, True)
    per = H.i3((1, 1, 1))
    oracle.sum_boundary_periodic(C.byref(f.view), H.i3((src_ng,) * 3), per, None)
    product.sum_boundary_periodic(C.byref(fd.view), H.i3((src_ng,) * 3), per, None)
    _sync(product)
    assert np.array_equal(fd.to_numpy(), f.to_numpy())


@pytest.mark.parametrize("names,ng_fill", [(("Ex", "Ey", "Ez", "Bx", "By", "Bz"), 2), (("Ex", "By"), 4), (("jx", "jy", "jz"), 1)])
def test_fill_boundary_of_several_fields_in_one_launch(oracle, product, names, ng_fill):
    """wxa_fill_boundary_periodic_multi (one launch per direction for all fields: E and B before the gather) against the
    oracle's fill of every field on its own: bit-identical, each staggering with its own boxes."""
    fs = H.random_fields(names, NCELL, 4, 61)
    fds = [f.copy_to(DEV, True) for f in fs]
    per = H.i3((1, 1, 1))
    for f in fs:
        oracle.fill_boundary_periodic(C.byref(f.view), H.i3((ng_fill,) * 3), per, None)
    views = (_capi.FieldView * len(fds))(*[f.view for f in fds])
    product.fill_boundary_periodic_multi(views, len(fds), H.i3((ng_fill,) * 3), per, None)
    _sync(product)
    for a, b in zip(fds, fs):
        assert np.array_equal(a.to_numpy(), b.to_numpy())
    with pytest.raises(_capi.WxaError):
        product.fill_boundary_periodic_multi(views, 7, H.i3((ng_fill,) * 3), per, None)


@pytest.mark.parametrize("src_ng", [2, 4])
def test_sum_boundary_of_several_fields_in_one_launch(oracle, product, src_ng):
    """wxa_sum_boundary_periodic_multi (the three components of J in SyncCurrent) against the oracle's sum per field."""
    fs = H.random_fields(("jx", "jy", "jz"), NCELL, 4, 71)
    fds = [f.copy_to(DEV, True) for f in fs]
    per = H.i3((1, 1, 0))
    for f in fs:
        oracle.sum_boundary_periodic(C.byref(f.view), H.i3((src_ng,) * 3), per, None)
    views = (_capi.FieldView * 3)(*[f.view for f in fds])
    product.sum_boundary_periodic_multi(views, 3, H.i3((src_ng,) * 3), per, None)
    _sync(product)
    for a, b in zip(fds, fs):
        assert np.array_equal(a.to_numpy(), b.to_numpy())


def test_field_set_zero_multi(product):
    """The three components of J zeroed by one launch (odd and even lengths, guards included); a fourth array is untouched."""
    fs = H.random_fields(("jx", "jy", "jz", "Ex"), (13, 8, 9), 3, 83)
    fds = [f.copy_to(DEV, True) for f in fs]
    views = (_capi.FieldView * 3)(*[f.view for f in fds[:3]])
    product.field_set_zero_multi(views, 3, None)
    _sync(product)
    for f in fds[:3]:
        assert not np.any(f.to_numpy())
    assert np.array_equal(fds[3].to_numpy(), fs[3].to_numpy())


def test_pack_unpack_roundtrip(product):
    import torch
    (f,) = H.random_fields(("Ey",), NCELL, 3, 80)
    fd = f.copy_to(DEV, True)
    lo = (C.c_int32 * 3)(-2, 1, 0)
    hi = (C.c_int32 * 3)(5, 9, 16)
    n = 7 * 8 * 16
    buf = torch.zeros(n, dtype=torch.float64, device=DEV)
    product.pack_box(C.byref(fd.view), lo, hi, buf.data_ptr(), None)
    a = f.to_numpy()
    want = a[-2 + 3:5 + 3, 1 + 3:9 + 3, 0 + 3:16 + 3]
    got = buf.cpu().numpy().reshape(16, 8, 7).transpose(2, 1, 0)
    assert np.array_equal(got, want)
    product.unpack_box(C.byref(fd.view), lo, hi, buf.data_ptr(), 1, None)
    _sync(product)
    b = fd.to_numpy()
    assert np.array_equal(b[-2 + 3:5 + 3, 1 + 3:9 + 3, 0 + 3:16 + 3], 2 * want)


def test_pack_unpack_f32_wire_against_the_oracle(oracle, product):
    """warpx.do_single_precision_comms: the slab rounded to float when packed, widened (and, for SumBoundary, added in
    double) when unpacked -- bit for bit what the oracle's host-side helpers do."""
    import torch
    (f,) = H.random_fields(("Ey",), NCELL, 3, 81)
    fd = f.copy_to(DEV, True)
    lo = (C.c_int32 * 3)(-2, 1, 0)
    hi = (C.c_int32 * 3)(5, 9, 16)
    n = 7 * 8 * 16
    buf = torch.zeros(n, dtype=torch.float32, device=DEV)
    ref = np.zeros(n, dtype=np.float32)
    product.pack_box_f32(C.byref(fd.view), lo, hi, buf.data_ptr(), None)
    oracle.pack_box_f32(C.byref(f.view), lo, hi, ref.ctypes.data, None)
    got = buf.cpu().numpy()
    assert np.array_equal(got, ref)
    assert not np.array_equal(got.astype(np.float64), f.to_numpy()[1:8, 4:12, 3:19].transpose(2, 1, 0).reshape(-1))   # it did round
    for mode in (1, 0):
        product.unpack_box_f32(C.byref(fd.view), lo, hi, buf.data_ptr(), mode, None)
        oracle.unpack_box_f32(C.byref(f.view), lo, hi, ref.ctypes.data, mode, None)
        _sync(product)
        assert np.array_equal(fd.to_numpy(), f.to_numpy())


def test_enforce_periodic_and_sort(oracle, product):
    import torch
    parts = H.random_particles(30000, NCELL, 90)
    # push some particles outside by up to one cell
    rng = np.random.default_rng(91)
    dx = H.LX / np.asarray(NCELL)
    for d in range(3):
        parts[d] = parts[d] + dx[d] * (rng.random(parts[d].shape[0]) - 0.5) * 2.0
    ph, pd = ParticleArrays.from_numpy(parts, "cpu"), ParticleArrays.from_numpy(parts, DEV)
    plo, phi = H.d3((-H.LX / 2,) * 3), H.d3((H.LX / 2,) * 3)
    per = H.i3((1, 1, 1))
    oracle.enforce_periodic(C.byref(ph.view), plo, phi, per, None)
    product.enforce_periodic(C.byref(pd.view), plo, phi, per, None)
    _sync(product)
    assert np.array_equal(pd.to_numpy(), ph.to_numpy())
    a = pd.to_numpy()
    assert np.all(a[:3] >= -H.LX / 2) and np.all(a[:3] < H.LX / 2)
    # counting sort by cell: a permutation whose cell ids are non-decreasing
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    out = ParticleArrays(pd.np, DEV)
    product.sort_particles_by_cell(C.byref(pd.view), C.byref(out.view), plo, H.d3(1.0 / dx),
                                   (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*NCELL), ws, None)
    _sync(product)
    s = out.to_numpy()
    cell = [np.clip(np.floor((s[d] + H.LX / 2) / dx[d]).astype(np.int64), 0, NCELL[d] - 1) for d in range(3)]
    T = 8  # tile-major cell key (WXA_TILE): tiles of 8^3 cells; inside a tile i, then parity of k, then j, then k//2
    nt = [(n + T - 1) // T for n in NCELL]
    tile = cell[0] // T + nt[0] * (cell[1] // T + nt[1] * (cell[2] // T))
    kt = cell[2] % T
    key = tile * T ** 3 + cell[0] % T + T * ((kt & 1) + 2 * (cell[1] % T + T * (kt >> 1)))
    assert np.all(np.diff(key) >= 0)
    order_a = np.lexsort(a[::-1])
    order_s = np.lexsort(s[::-1])
    assert np.array_equal(a[:, order_a], s[:, order_s])
    product.workspace_destroy(ws)


@pytest.mark.parametrize("drift,retire", [(0.0, False), (0.3, False), (0.3, True), (3.0, False)])
def test_sort_of_a_nearly_sorted_tile(product, drift, retire, monkeypatch):
    """The windowed scatter (a workgroup stages the particles that stay near their place in LDS and writes whole
    lines) on what it is built for -- a second sort after the particles drifted by a fraction of a cell -- and on what it
    must survive: no drift at all, a drift of several cells (most particles beyond the window margin), retired particles
    (sorted behind the live ones).  Keys non-decreasing, every particle once, ids with their particles; two sorts of the
    same input give the same tile."""
    ncell = (24, 16, 40)
    n = 150000
    parts = H.random_particles(n, ncell, 95)
    rng = np.random.default_rng(96)
    dx = H.LX / np.asarray(ncell)
    plo = H.d3((-H.LX / 2,) * 3)
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    ids = np.arange(1, n + 1, dtype=np.int64)
    first = ParticleArrays.from_numpy(parts, DEV, ids)
    srt = ParticleArrays(n, DEV, with_id=True)
    args = (plo, H.d3(1.0 / dx), (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*ncell), ws, None)
    product.sort_particles_by_cell(C.byref(first.view), C.byref(srt.view), *args)
    _sync(product)
    a = srt.to_numpy()
    aid = srt.ids_to_numpy()
    for d in range(3):   # drift, kept inside the box
        a[d] = np.clip(a[d] + drift * dx[d] * rng.standard_normal(n), -H.LX / 2 * 0.999, H.LX / 2 * 0.999)
    if retire:
        gone = rng.random(n) < 0.01
        aid = np.where(gone, np.int64(-1), aid)       # WXA_IDCPU_RETIRED = all ones
        a[3] = np.where(gone, 0.0, a[3])
    results = []
    for mode in ("0", "1"):
        src = ParticleArrays.from_numpy(list(a), DEV, aid)
        out = ParticleArrays(n, DEV, with_id=True)
        product.sort_particles_by_cell(C.byref(src.view), C.byref(out.view), *args)
        _sync(product)
        s, sid = out.to_numpy(), out.ids_to_numpy()
        live = sid != -1
        assert live.sum() == (aid != -1).sum() and np.all(live[:live.sum()])      # retired ones at the end
        sl = s[:, live]
        cell = [np.clip(np.floor((sl[d] + H.LX / 2) / dx[d]).astype(np.int64), 0, ncell[d] - 1) for d in range(3)]
        T = 8
        nt = [(m + T - 1) // T for m in ncell]
        tile = cell[0] // T + nt[0] * (cell[1] // T + nt[1] * (cell[2] // T))
        kt = cell[2] % T
        key = tile * T ** 3 + cell[0] % T + T * ((kt & 1) + 2 * (cell[1] % T + T * (kt >> 1)))
        assert np.all(np.diff(key) >= 0)
        order = np.argsort(sid[live], kind="stable")
        results.append((sid[live][order], sl[:, order]))
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    ref_order = np.argsort(aid[aid != -1], kind="stable")
    assert np.array_equal(results[1][1], a[:, aid != -1][:, ref_order])           # every particle arrived with its own data
    product.workspace_destroy(ws)


@pytest.mark.parametrize("steps", [0, 3, 6, 7])
def test_enforce_periodic_through_the_sort(product, steps):
    """wxa_enforce_periodic_sorted (face tiles of the last sort + appended tail) against the plain pass, bit for bit:
    particles displaced by up to `steps` cells since the sort, an unsorted tail behind them."""
    import torch
    ncell = (24, 20, 16)
    dx = H.LX / np.asarray(ncell)
    parts = H.random_particles(50000, ncell, 77, u_scale=0.1)
    pd0 = ParticleArrays.from_numpy(parts, DEV)
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    big = ParticleArrays(pd0.np + 5000, DEV)       # room for a tail behind the sorted part
    srt_view = big.view
    srt_view.np = pd0.np
    product.sort_particles_by_cell(C.byref(pd0.view), C.byref(srt_view), H.d3((-H.LX / 2,) * 3), H.d3(1.0 / dx),
                                   (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*ncell), ws, None)
    _sync(product)
    rng = np.random.default_rng(8)
    for d in range(3):
        big.data[d][:pd0.np] += torch.from_numpy(dx[d] * max(steps, 0.5) * (2 * rng.random(pd0.np) - 1)).to(DEV)
        big.data[d][pd0.np:] = torch.from_numpy(H.LX * (1.5 * rng.random(5000) - 0.75)).to(DEV)   # tail: anywhere within one period
    ref = ParticleArrays(big.np, DEV)
    ref.data.copy_(big.data)
    per = (C.c_int * 3)(1, 1, 0)
    lo, hi = H.d3((-H.LX / 2,) * 3), H.d3((H.LX / 2,) * 3)
    product.enforce_periodic(C.byref(ref.view), lo, hi, per, None)
    product.enforce_periodic_sorted(C.byref(big.view), lo, hi, per, ws, steps, None)
    _sync(product)
    assert torch.equal(big.data, ref.data)
    a = ref.to_numpy()
    assert np.all(a[0] >= -H.LX / 2) and np.all(a[0] < H.LX / 2) and np.all(a[1] >= -H.LX / 2) and np.all(a[1] < H.LX / 2)
    product.workspace_destroy(ws)


@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("algo", [_capi.DEPOSIT_ESIRKEPOV, _capi.DEPOSIT_DIRECT])
@pytest.mark.parametrize("stale", [False, True])
@pytest.mark.parametrize("u_scale", [1.0, 0.003])
def test_deposit_current_lds_tiles(oracle, product, order, algo, stale, u_scale):
    """LDS-tile variant (needs a cell sort in the workspace) against the oracle; `stale` moves the
    particles by up to 0.9 cell after the sort (and outside the domain) so that part of the
    stencils leave their tile and take the global-atomic path."""
    ncell = (24, 20, 16)
    _, ng_depos, ng_j = H.guard_depths(order, use_filter=True)
    # u_scale = 1: most particles cross a cell (general path); 0.003: almost none (fast path)
    parts = H.random_particles(40000, ncell, 200 + order, u_scale=u_scale)
    dx = H.LX / np.asarray(ncell)
    pd0 = ParticleArrays.from_numpy(parts, DEV)
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    srt = ParticleArrays(pd0.np, DEV)
    product.sort_particles_by_cell(C.byref(pd0.view), C.byref(srt.view), H.d3((-H.LX / 2,) * 3), H.d3(1.0 / dx),
                                   (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*ncell), ws, None)
    _sync(product)
    if stale:
        rng = np.random.default_rng(5)
        for d in range(3):
            srt.data[d] += __import__("torch").from_numpy(dx[d] * 0.9 * (2 * rng.random(srt.np) - 1)).to(DEV)
    ph = ParticleArrays.from_numpy(list(srt.to_numpy()), "cpu")
    J = [FieldArray(ncell, STAG[n], (ng_j,) * 3, "cpu") for n in ("jx", "jy", "jz")]
    Jd = H.clone_fields(J, DEV, True)
    g, _ = H.geom_for(ncell, ng_depos)
    dt = H.yee_dt(dx)
    q = -plasma.Q_E
    oracle.deposit_current(C.byref(ph.view), field_triplet(J), C.byref(g), q, dt, -0.5 * dt, order, algo, None, None)
    product.deposit_current(C.byref(srt.view), field_triplet(Jd), C.byref(g), q, dt, -0.5 * dt, order, algo, ws, None)
    _sync(product)
    # slow particles: J is a difference of nearly equal shape weights (S_new - S_old ~ 1e-3 S), so
    # the summation-order rounding is amplified by ~1/u_scale; still far inside the 1e-10 gate
    tol = 1e-12 if u_scale == 1.0 else 2e-11
    for a, b in zip(Jd, J):
        assert H.max_rel_err(a.to_numpy(), b.to_numpy()) < tol
    product.workspace_destroy(ws)


@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("algo", [_capi.DEPOSIT_ESIRKEPOV, _capi.DEPOSIT_DIRECT])
@pytest.mark.parametrize("drift", [0.0, 2.5])
@pytest.mark.parametrize("heavy", [None, 1500])
def test_deposit_current_lds_tiles_crowded_cells(oracle, product, order, algo, drift, heavy, monkeypatch):
    """Cells with more particles than the tile kernel's work items cover (more than 24 in a cell: at 8 per cell on
    average about one cell in a million, i.e. only at the headline size -- found there, round 3, by
    test_direct_vay_ckc_256_against_the_oracle: the overflow list was deposited with the Esirkepov body whatever the
    algorithm).  A few cells with 30 to 90 particles among ordinary ones, both algorithms, against the oracle.
    drift: every particle moved by up to that many cells after the sort.  The particles of a crowded cell beyond the
    24th reach the deposition by index only, unseen by the chunk loop and its range check -- until round 5 their wide
    frame was written to the LDS tile wherever it lay, and a frame outside the tile overwrote the lists next to it in
    LDS (found by the boosted wakefield deck at 8 particles per cell: a density spike, electrons moving a cell per step,
    a memory fault on the MI355X; reproduced on the CPU execution model with guard pages).
    heavy: WXA_HEAVY_TILE, the particle count beyond which a tile is shared by several workgroups (csrc/heavy_tiles.hpp;
    32768 by default): at 1500 the tiles of the spike and of the other crowded cells are split into two to four units."""
    if heavy is not None:
        monkeypatch.setenv("WXA_HEAVY_TILE", str(heavy))
    ncell = (16, 16, 16)
    _, ng_depos, ng_j = H.guard_depths(order, use_filter=True)
    parts = H.random_particles(20000, ncell, 77 + order, u_scale=1.0)
    dx = H.LX / np.asarray(ncell)
    rng = np.random.default_rng(12)
    crowd = []
    # ... and one cell like a wake's density spike: thousands of particles, which leave the tile kernel for the
    # global-atomics pass as one block of the straggler list
    for cell, count in (((3, 4, 5), 30), ((8, 8, 8), 57), ((15, 0, 7), 90), ((9, 8, 8), 26), ((5, 9, 2), 3000), ((6, 9, 2), 70)):
        pos = [-H.LX / 2 + (cell[d] + rng.random(count)) * dx[d] for d in range(3)]
        crowd.append(pos + [1e9 * (0.5 + rng.random(count))] + [plasma.C_LIGHT * rng.standard_normal(count) for _ in range(3)])
    parts = [np.concatenate([parts[r]] + [c[r] for c in crowd]) for r in range(7)]
    pd0 = ParticleArrays.from_numpy(parts, DEV)
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    srt = ParticleArrays(pd0.np, DEV)
    product.sort_particles_by_cell(C.byref(pd0.view), C.byref(srt.view), H.d3((-H.LX / 2,) * 3), H.d3(1.0 / dx),
                                   (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*ncell), ws, None)
    _sync(product)
    if drift:
        import torch
        for d in range(3):
            srt.data[d] += torch.from_numpy(dx[d] * drift * (2 * rng.random(srt.np) - 1)).to(DEV)
            srt.data[d].clamp_(-H.LX / 2 + 0.01 * dx[d], H.LX / 2 - 0.01 * dx[d])
    ph = ParticleArrays.from_numpy(list(srt.to_numpy()), "cpu")
    J = [FieldArray(ncell, STAG[n], (ng_j,) * 3, "cpu") for n in ("jx", "jy", "jz")]
    Jd = H.clone_fields(J, DEV, True)
    g, _ = H.geom_for(ncell, ng_depos)
    dt = H.yee_dt(dx)
    q = -plasma.Q_E
    oracle.deposit_current(C.byref(ph.view), field_triplet(J), C.byref(g), q, dt, -0.5 * dt, order, algo, None, None)
    product.deposit_current(C.byref(srt.view), field_triplet(Jd), C.byref(g), q, dt, -0.5 * dt, order, algo, ws, None)
    _sync(product)
    for a, b in zip(Jd, J):
        assert H.max_rel_err(a.to_numpy(), b.to_numpy()) < 1e-12
    product.workspace_destroy(ws)


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("streaming", [0, 1])
@pytest.mark.parametrize("drift", [0.0, 0.8])
@pytest.mark.parametrize("spike", [0, 3000])
@pytest.mark.parametrize("n", [4000, 60000, 160000])
def test_deposit_current_of_a_streaming_plasma(oracle, product, order, streaming, drift, spike, n):
    """A plasma that streams through the grid (a boosted-frame run: every particle moves 0.76 cells per step against the
    boost, three in four cross a cell) on the LDS tiles, against the oracle: with wxa_workspace_set_streaming_plasma every
    particle goes through the wide-frame body inside the tile loop; without it the crossing particles go through the
    deferred list and, what it cannot take (most of them here), the global-atomics pass -- the same J either way.
    drift: moved by up to that many cells after the sort.
    spike: that many particles in ONE cell and a tenth of it in its neighbour (a wake's density spike): with the streaming
    body the lanes of a wave that share a frame sum every value over the wave before one lane adds it (wave_sum_f64).
    n: 0.65, 10 and 26 particles per cell on average; at 26 the pairs beyond a cell's fourth do not fit the tile's tail
    table and all of them become excess chunks; at 0.65 (a sparse tile, with the streaming body) all pairs go through the
    table and the direct part's chunks are skipped -- with the spike, one tile is sparse but for a cell of thousands."""
    ncell = (16, 16, 24)
    _, ng_depos, ng_j = H.guard_depths(order, use_filter=True)
    parts = H.random_particles(n, ncell, 410 + order, u_scale=0.05)
    dx = H.LX / np.asarray(ncell)
    if spike:
        rng = np.random.default_rng(77)
        crowd = []
        for cell, count in (((5, 9, 11), spike), ((6, 9, 11), spike // 10), ((12, 3, 17), 150)):
            pos = [-H.LX / 2 + (cell[d] + rng.random(count)) * dx[d] for d in range(3)]
            crowd.append(pos + [1e9 * (0.5 + rng.random(count))] + [0.05 * plasma.C_LIGHT * rng.standard_normal(count) for _ in range(3)])
        parts = [np.concatenate([parts[r]] + [c[r] for c in crowd]) for r in range(7)]
    dt = H.yee_dt(dx)
    beta = 0.76 * dx[2] / (plasma.C_LIGHT * dt)           # v dt = 0.76 dz along -z
    beta = min(beta, 0.98)
    parts[6] = parts[6] - beta / np.sqrt(1.0 - beta ** 2) * plasma.C_LIGHT
    pd0 = ParticleArrays.from_numpy(parts, DEV)
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    product.workspace_set_streaming_plasma(ws, streaming)
    srt = ParticleArrays(pd0.np, DEV)
    product.sort_particles_by_cell(C.byref(pd0.view), C.byref(srt.view), H.d3((-H.LX / 2,) * 3), H.d3(1.0 / dx),
                                   (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*ncell), ws, None)
    _sync(product)
    if drift:
        import torch
        rng = np.random.default_rng(9)
        for d in range(3):
            srt.data[d] += torch.from_numpy(dx[d] * drift * (2 * rng.random(srt.np) - 1)).to(DEV)
            srt.data[d].clamp_(-H.LX / 2 + 0.01 * dx[d], H.LX / 2 - 0.01 * dx[d])
    ph = ParticleArrays.from_numpy(list(srt.to_numpy()), "cpu")
    J = [FieldArray(ncell, STAG[n], (ng_j,) * 3, "cpu") for n in ("jx", "jy", "jz")]
    Jd = H.clone_fields(J, DEV, True)
    g, _ = H.geom_for(ncell, ng_depos)
    q = -plasma.Q_E
    oracle.deposit_current(C.byref(ph.view), field_triplet(J), C.byref(g), q, dt, -0.5 * dt, order, _capi.DEPOSIT_ESIRKEPOV, None, None)
    product.deposit_current(C.byref(srt.view), field_triplet(Jd), C.byref(g), q, dt, -0.5 * dt, order, _capi.DEPOSIT_ESIRKEPOV, ws, None)
    _sync(product)
    for a, b in zip(Jd, J):
        assert H.max_rel_err(a.to_numpy(), b.to_numpy()) < 1e-12
    product.workspace_destroy(ws)


@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("keep", [1.0, 0.7, 0.4, 0.12])
@pytest.mark.parametrize("step_cells", [0.76, 0.5])
def test_deposit_current_of_a_cold_stream_on_a_lattice(oracle, product, order, keep, step_cells):
    """The plasma ahead of a boosted-frame wake: eight particles per cell on a 2 x 2 x 2 lattice, cold, every one of them
    `step_cells` of a cell along -z per step.  At 0.76 all of them cross a cell face and the pairs of a cell share their
    wide frame: whole waves take the streaming body's PairScatterSink (lanes l and l + 32 share the summing AND the
    adding); at 0.5 half of a cell's particles cross and the lane pairs' frames differ (PairSumSink).  keep < 1: that
    share of the particles, at random -- cells with odd counts, lanes and lane pairs without a particle; at 0.4 and 0.12 a
    tile holds ~1600 / ~500 particles and lists all its pairs in the table instead of running the direct part's chunks."""
    ncell = (16, 16, 24)
    _, ng_depos, ng_j = H.guard_depths(order, use_filter=True)
    dx = H.LX / np.asarray(ncell)
    ax = [-H.LX / 2 + (np.arange(2 * ncell[d]) + 0.5) * dx[d] / 2 for d in range(3)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    rng = np.random.default_rng(5)
    sel = rng.random(X.size) < keep
    n = int(sel.sum())
    dt = H.yee_dt(dx)
    beta = min(step_cells * dx[2] / (plasma.C_LIGHT * dt), 0.98)
    parts = [X.ravel()[sel], Y.ravel()[sel], Z.ravel()[sel], 1e9 * (0.5 + rng.random(n)),
             np.zeros(n), np.zeros(n), np.full(n, -beta / np.sqrt(1.0 - beta ** 2) * plasma.C_LIGHT)]
    pd0 = ParticleArrays.from_numpy(parts, DEV)
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    product.workspace_set_streaming_plasma(ws, 1)
    srt = ParticleArrays(pd0.np, DEV)
    product.sort_particles_by_cell(C.byref(pd0.view), C.byref(srt.view), H.d3((-H.LX / 2,) * 3), H.d3(1.0 / dx),
                                   (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*ncell), ws, None)
    _sync(product)
    ph = ParticleArrays.from_numpy(list(srt.to_numpy()), "cpu")
    J = [FieldArray(ncell, STAG[n], (ng_j,) * 3, "cpu") for n in ("jx", "jy", "jz")]
    Jd = H.clone_fields(J, DEV, True)
    g, _ = H.geom_for(ncell, ng_depos)
    q = -plasma.Q_E
    # the positions handed over are the ones after the push (the deposition steps back by v dt): inside the box either way
    oracle.deposit_current(C.byref(ph.view), field_triplet(J), C.byref(g), q, dt, -0.5 * dt, order, _capi.DEPOSIT_ESIRKEPOV, None, None)
    product.deposit_current(C.byref(srt.view), field_triplet(Jd), C.byref(g), q, dt, -0.5 * dt, order, _capi.DEPOSIT_ESIRKEPOV, ws, None)
    _sync(product)
    for a, b in zip(Jd, J):
        assert H.max_rel_err(a.to_numpy(), b.to_numpy()) < 1e-12
    product.workspace_destroy(ws)


@pytest.mark.parametrize("algo,acc", [(_capi.DEPOSIT_ESIRKEPOV, _capi.ACC_FP64), (_capi.DEPOSIT_DIRECT, _capi.ACC_FP64),
                                      (_capi.DEPOSIT_ESIRKEPOV, _capi.ACC_FP32)])
@pytest.mark.parametrize("ppc", [20, 40])
def test_deposit_current_lds_tiles_many_particles_per_cell(oracle, product, algo, acc, ppc):
    """20 and 40 particles per cell on average (the tile kernel's tables are sized for 8: the tail table of a tile holds
    1024 pairs beyond the fourth of a cell, the deferred list 2048 particles; what does not fit goes on to the next list
    and finally to the global-atomics kernel) -- every overflow path at once, order 3, against the oracle."""
    order = 3
    ncell = (16, 16, 8)
    _, ng_depos, ng_j = H.guard_depths(order, use_filter=True)
    parts = H.random_particles(ppc * ncell[0] * ncell[1] * ncell[2], ncell, 31 + ppc, u_scale=1.0)
    dx = H.LX / np.asarray(ncell)
    pd0 = ParticleArrays.from_numpy(parts, DEV)
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    product.workspace_set_deposit_accumulator(ws, acc)
    srt = ParticleArrays(pd0.np, DEV)
    product.sort_particles_by_cell(C.byref(pd0.view), C.byref(srt.view), H.d3((-H.LX / 2,) * 3), H.d3(1.0 / dx),
                                   (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*ncell), ws, None)
    _sync(product)
    ph = ParticleArrays.from_numpy(list(srt.to_numpy()), "cpu")
    J = [FieldArray(ncell, STAG[n], (ng_j,) * 3, "cpu") for n in ("jx", "jy", "jz")]
    Jd = H.clone_fields(J, DEV, True)
    g, _ = H.geom_for(ncell, ng_depos)
    dt = H.yee_dt(dx)
    q = -plasma.Q_E
    oracle.deposit_current(C.byref(ph.view), field_triplet(J), C.byref(g), q, dt, -0.5 * dt, order, algo, None, None)
    product.deposit_current(C.byref(srt.view), field_triplet(Jd), C.byref(g), q, dt, -0.5 * dt, order, algo, ws, None)
    _sync(product)
    for a, b in zip(Jd, J):   # fp32 tiles: the reference's single-precision gate (test_deposit_current_fp32_tiles)
        assert H.max_rel_err(a.to_numpy(), b.to_numpy()) < (1e-12 if acc == _capi.ACC_FP64 else 2e-6)
    product.workspace_destroy(ws)


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("zero_dir", [0, 1, 2])
@pytest.mark.parametrize("u_scale", [0.003, 1.0])
def test_esirkepov_zero_displacement_deposits_exactly_zero(product, order, zero_dir, u_scale):
    """A particle with u_d == 0 has x_old == x_new bit for bit in the reference (CurrentDeposition.H:700-716), so its
    old and new weights are identical and sdxi = (sx_old - sx_new) * ... of :792-801 is exactly 0: J_d == 0.0 on every
    point (the antenna particles of test_3d_laser_injection.json, jx golden value 0.0, comparator atol 0).  Checked on
    the global-atomics kernel and on the LDS-tile kernel (fast pairs / singles at small u, general path at large u)."""
    ncell = (24, 20, 16)
    _, ng_depos, ng_j = H.guard_depths(order, use_filter=True)
    parts = H.random_particles(30000, ncell, 900 + order, u_scale=u_scale)
    parts[4 + zero_dir][:] = 0.0
    # several particles per cell so that the tile kernel forms pairs
    for d in range(3):
        parts[d][10000:20000] = parts[d][:10000] + 1e-3 * (H.LX / ncell[d])
    parts[4 + zero_dir][:] = 0.0
    dx = H.LX / np.asarray(ncell)
    g, _ = H.geom_for(ncell, ng_depos)
    dt = H.yee_dt(dx)
    q = -plasma.Q_E
    pd0 = ParticleArrays.from_numpy(parts, DEV)
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    srt = ParticleArrays(pd0.np, DEV)
    product.sort_particles_by_cell(C.byref(pd0.view), C.byref(srt.view), H.d3((-H.LX / 2,) * 3), H.d3(1.0 / dx),
                                   (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*ncell), ws, None)
    for use_ws, pa in ((None, pd0), (ws, srt)):
        for rel_t in (-0.5 * dt, 0.0):
            Jd = [FieldArray(ncell, STAG[n], (ng_j,) * 3, DEV, pad=True) for n in ("jx", "jy", "jz")]
            product.deposit_current(C.byref(pa.view), field_triplet(Jd), C.byref(g), q, dt, rel_t, order,
                                    _capi.DEPOSIT_ESIRKEPOV, use_ws, None)
            _sync(product)
            j = [f.to_numpy() for f in Jd]
            assert np.count_nonzero(j[zero_dir]) == 0, (use_ws is not None, rel_t, float(np.max(np.abs(j[zero_dir]))))
            assert all(np.max(np.abs(j[d])) > 0 for d in range(3) if d != zero_dir)
    product.workspace_destroy(ws)


@pytest.mark.parametrize("stale", [False, True])
@pytest.mark.parametrize("u_scale", [1.0, 0.003])
def test_deposit_tiles_fast_and_crossing_paths(oracle, product, stale, u_scale):
    """The order-3 LDS-tile depositions (Esirkepov and direct) against the oracle: fresh and stale sort, a plasma where
    nearly every particle stays in its cell (pair body) and one where most cross (wide-frame body); and exact zeros."""
    test_deposit_current_lds_tiles(oracle, product, 3, _capi.DEPOSIT_ESIRKEPOV, stale, u_scale)
    test_deposit_current_lds_tiles(oracle, product, 3, _capi.DEPOSIT_DIRECT, stale, u_scale)
    if not stale:
        test_esirkepov_zero_displacement_deposits_exactly_zero(product, 3, 1, u_scale)


@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("u_scale", [1.0, 0.01])
def test_deposit_current_fp32_tiles(oracle, product, order, u_scale):
    """The ds_add_f32 variant of the LDS-tile Esirkepov deposition (wxa_workspace_set_deposit_accumulator, WXA_ACC_FP32)
    against the fp64 oracle at the reference's single-precision tolerance, 2e-6 of max|J|
    (Examples/analysis_default_regression.py:18), and charge conservation at the same level: the values are computed in
    fp64 and rounded once on entering the tile, so only the tile's sums carry fp32 round-off."""
    ncell = (24, 20, 16)
    _, ng_depos, ng_j = H.guard_depths(order, use_filter=True)
    parts = H.random_particles(60000, ncell, 300 + order, u_scale=u_scale)
    dx = H.LX / np.asarray(ncell)
    pd0 = ParticleArrays.from_numpy(parts, DEV)
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    product.workspace_set_deposit_accumulator(ws, _capi.ACC_FP32)
    srt = ParticleArrays(pd0.np, DEV)
    product.sort_particles_by_cell(C.byref(pd0.view), C.byref(srt.view), H.d3((-H.LX / 2,) * 3), H.d3(1.0 / dx),
                                   (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*ncell), ws, None)
    _sync(product)
    ph = ParticleArrays.from_numpy(list(srt.to_numpy()), "cpu")
    J = [FieldArray(ncell, STAG[n], (ng_j,) * 3, "cpu") for n in ("jx", "jy", "jz")]
    Jd = H.clone_fields(J, DEV, True)
    g, _ = H.geom_for(ncell, ng_depos)
    dt = H.yee_dt(dx)
    q = -plasma.Q_E
    oracle.deposit_current(C.byref(ph.view), field_triplet(J), C.byref(g), q, dt, -0.5 * dt, order,
                           _capi.DEPOSIT_ESIRKEPOV, None, None)
    product.deposit_current(C.byref(srt.view), field_triplet(Jd), C.byref(g), q, dt, -0.5 * dt, order,
                            _capi.DEPOSIT_ESIRKEPOV, ws, None)
    _sync(product)
    errs = [H.max_rel_err(a.to_numpy(), b.to_numpy()) for a, b in zip(Jd, J)]
    print("fp32 tiles: max |dJ| / max|J| per component", errs)
    assert max(errs) < 2e-6
    assert max(errs) > 1e-12   # really the fp32 path
    product.workspace_destroy(ws)


@pytest.mark.parametrize("order,galerkin,pusher", [(1, 1, _capi.PUSHER_BORIS), (2, 1, _capi.PUSHER_BORIS), (3, 1, _capi.PUSHER_BORIS),
                                                   (3, 0, _capi.PUSHER_BORIS), (2, 0, _capi.PUSHER_BORIS), (1, 0, _capi.PUSHER_BORIS),
                                                   (3, 1, _capi.PUSHER_VAY), (3, 0, _capi.PUSHER_VAY), (2, 1, _capi.PUSHER_VAY),
                                                   (3, 1, _capi.PUSHER_HC), (1, 0, _capi.PUSHER_HC),
                                                   # order 4 on the tiles (round 6): 13^3 / 14^3 staged points
                                                   (4, 1, _capi.PUSHER_BORIS), (4, 0, _capi.PUSHER_BORIS), (4, 1, _capi.PUSHER_VAY)])
@pytest.mark.parametrize("stale", [False, True])
@pytest.mark.parametrize("heavy", [None, 700])
def test_gather_push_lds_tiles(oracle, product, order, galerkin, pusher, stale, heavy, monkeypatch):
    """LDS-tile gather (needs a cell sort in the workspace) against the oracle; `stale` moves the
    particles after the sort so that some stencils leave the staged range (global-load path).  Boris, Vay and
    Higuera-Cary on the tile kernel itself (until round 5 the other pushers met it only through the step tests).
    heavy: WXA_HEAVY_TILE = 700 shares every tile of more than 700 particles (most of them here: 2000 on average) between
    several workgroups, each with a part of the tile's particles (csrc/heavy_tiles.hpp)."""
    if heavy is not None:
        monkeypatch.setenv("WXA_HEAVY_TILE", str(heavy))
    import torch
    ncell = (24, 20, 16)
    ng, _, _ = H.guard_depths(order)
    E = H.random_fields(("Ex", "Ey", "Ez"), ncell, ng, 10, scale=1e11)
    B = H.random_fields(("Bx", "By", "Bz"), ncell, ng, 11, scale=1e3)
    Ed, Bd = H.clone_fields(E, DEV, True), H.clone_fields(B, DEV, True)
    parts = H.random_particles(30000, ncell, 300 + order)
    dx = H.LX / np.asarray(ncell)
    pd0 = ParticleArrays.from_numpy(parts, DEV)
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    srt = ParticleArrays(pd0.np, DEV)
    product.sort_particles_by_cell(C.byref(pd0.view), C.byref(srt.view), H.d3((-H.LX / 2,) * 3), H.d3(1.0 / dx),
                                   (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*ncell), ws, None)
    _sync(product)
    if stale:
        rng = np.random.default_rng(6)
        for d in range(3):
            srt.data[d] += torch.from_numpy(dx[d] * 0.9 * (2 * rng.random(srt.np) - 1)).to(DEV)
            # keep the particles inside the domain, as the step loop guarantees at gather time
            srt.data[d].clamp_(-H.LX / 2, H.LX / 2 - 1e-12)
    ph = ParticleArrays.from_numpy(list(srt.to_numpy()), "cpu")
    g, _ = H.geom_for(ncell, ng)
    dt = H.yee_dt(dx)
    q, m = -plasma.Q_E, plasma.M_E
    for move, fn in ((1, "gather_push"), (0, "push_p")):
        getattr(oracle, fn)(C.byref(ph.view), field_triplet(E), field_triplet(B), C.byref(g), q, m, dt,
                            order, galerkin, pusher, None)
        product.gather_push_ws(C.byref(srt.view), field_triplet(Ed), field_triplet(Bd), C.byref(g), q, m, dt,
                               order, galerkin, pusher, move, ws, None)
        _sync(product)
        a, b = srt.to_numpy(), ph.to_numpy()
        for row in range(7):
            assert H.max_rel_err(a[row], b[row]) < 1e-12, (fn, row)
    product.workspace_destroy(ws)


def _tile_major_key(pos, ncell, dx, wrap):
    """cell_of (csrc/push_sort.hpp) in numpy: the tile-major cell key, indices one period outside brought back where
    `wrap` says so, clamped otherwise."""
    cell = []
    for d in range(3):
        c = np.floor((pos[d] + H.LX / 2) / dx[d]).astype(np.int64)
        if wrap[d]:
            c = np.where(c < 0, c + ncell[d], np.where(c >= ncell[d], c - ncell[d], c))
        cell.append(np.clip(c, 0, ncell[d] - 1))
    T = 8
    nt = [(m + T - 1) // T for m in ncell]
    tile = cell[0] // T + nt[0] * (cell[1] // T + nt[1] * (cell[2] // T))
    kt = cell[2] % T
    return tile * T ** 3 + cell[0] % T + T * ((kt & 1) + 2 * (cell[1] % T + T * (kt >> 1)))


@pytest.mark.parametrize("order,sort_first,tail,retire,every_step,predict", [
    (3, True, 0, False, False, False),     # the LDS-tile kernels (tile + stragglers)
    (3, True, 0, False, False, True),      # ... keyed one free-flight step ahead (what the host layer does)
    (3, True, 700, True, False, True),     # ... with an appended tail (global-memory kernel), retired particles, arrivals after the count
    (1, True, 0, True, True, False),       # COUNT and SCATTER in the same push (a sort every step)
    (4, False, 0, False, False, True),     # no tiles at all: the global-memory kernel does everything
    (2, True, 300, False, True, False),
    (3, True, 700, True, False, "heavy"),  # tiles shared by several workgroups (WXA_HEAVY_TILE): unit 0 counts in LDS, the others globally
])
def test_sort_folded_into_the_push(oracle, product, order, sort_first, tail, retire, every_step, predict, monkeypatch):
    """wxa_push_sort_begin / _end (SortParticlesByBin folded into PushPX, csrc/push_sort.hpp): three pushes, the first
    records keys and ranks (COUNT), the second writes the particles into the sorted tile (SCATTER), the third runs on
    that tile through the workspace the SCATTER left.  Against the oracle's plain pushes of the same particles: every
    particle arrives with its own data (ids), pushed to 1e-12; the new order is the tile-major cell order of the
    positions BEFORE the scattering push, wrapped along the periodic directions -- or, with predict_dt, of those positions
    carried one time step further in free flight (x + u / gamma dt); retired particles of the record end up behind
    everything and are dropped; particles appended after the COUNT follow the cell-sorted ones in their order."""
    import torch
    if predict == "heavy":
        monkeypatch.setenv("WXA_HEAVY_TILE", "900")
        predict = True
    ncell = (24, 20, 16)
    ng, _, _ = H.guard_depths(order)
    E = H.random_fields(("Ex", "Ey", "Ez"), ncell, ng, 10, scale=1e11)
    B = H.random_fields(("Bx", "By", "Bz"), ncell, ng, 11, scale=1e3)
    Ed, Bd = H.clone_fields(E, DEV, True), H.clone_fields(B, DEV, True)
    n0, n_arrive = 30000, 400
    parts = H.random_particles(n0 + tail, ncell, 500 + order, u_scale=30.0)   # up to ~0.5 cell per push
    dx = H.LX / np.asarray(ncell)
    plo, dinv = H.d3((-H.LX / 2,) * 3), H.d3(1.0 / dx)
    lo, nc = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*ncell)
    wrap_flags = (1, 0, 1)
    wrap = (C.c_int32 * 3)(*wrap_flags)
    g, _ = H.geom_for(ncell, ng)
    dt = H.yee_dt(dx)
    q, m = -plasma.Q_E, plasma.M_E
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    cap = n0 + tail + n_arrive
    ids0 = np.arange(1, n0 + tail + 1, dtype=np.int64)
    cur = ParticleArrays(cap, DEV, with_id=True)          # the tile, with room for arrivals
    head = [np.asarray(r[:n0]) for r in parts]
    if sort_first:   # a classic sort of the first n0 particles; `tail` more are appended behind it
        src = ParticleArrays.from_numpy(head, DEV, ids0[:n0])
        v = cur.view
        v.np = n0
        product.sort_particles_by_cell(C.byref(src.view), C.byref(v), plo, dinv, lo, nc, ws, None)
        _sync(product)
        for r in range(7):
            cur.data[r][n0:n0 + tail] = torch.from_numpy(np.asarray(parts[r][n0:])).to(DEV)
        cur.idcpu[n0:n0 + tail] = torch.from_numpy(ids0[n0:]).to(DEV)
    else:
        for r in range(7):
            cur.data[r][:n0 + tail] = torch.from_numpy(np.asarray(parts[r])).to(DEV)
        cur.idcpu[:n0 + tail] = torch.from_numpy(ids0).to(DEV)
    npart = n0 + tail
    rng = np.random.default_rng(17)

    def view_of(pa, n):
        v = pa.view
        v.np = n
        return v

    def host_copy(pa, n):
        return pa.to_numpy()[:, :n], pa.ids_to_numpy()[:n]

    def oracle_push(rows):
        ph = ParticleArrays.from_numpy(list(rows), "cpu")
        oracle.gather_push(C.byref(ph.view), field_triplet(E), field_triplet(B), C.byref(g), q, m, dt, order, 1,
                           _capi.PUSHER_BORIS, None)
        return ph.to_numpy()

    def keep_inside(pa, n):   # what Redistribute does between two pushes: periodic wrap, or a wall that keeps them in
        for d in range(3):
            x = pa.data[d][:n]
            if wrap_flags[d]:
                x.copy_(torch.where(x >= H.LX / 2, x - H.LX, torch.where(x < -H.LX / 2, x + H.LX, x)))
            else:
                x.clamp_(-H.LX / 2, H.LX / 2 - 1e-12)

    live_i64 = C.c_int64()
    app_i64 = C.c_int64()
    spare = ParticleArrays(cap, DEV, with_id=True)
    modes = [_capi.PUSH_SORT_COUNT, _capi.PUSH_SORT_SCATTER | (_capi.PUSH_SORT_COUNT if every_step else 0),
             _capi.PUSH_SORT_SCATTER if every_step else 0]
    n_retired_in_record = 0
    for step, mode in enumerate(modes):
        before, before_ids = host_copy(cur, npart)
        want = oracle_push(before)
        pv, dv = view_of(cur, npart), view_of(spare, npart)
        if mode:
            assert (product.push_sort_pending(ws, C.byref(pv)) == 1) == bool(mode & _capi.PUSH_SORT_SCATTER)
            rc = product.push_sort_begin(ws, mode, C.byref(pv), C.byref(dv), plo, dinv, lo, nc, wrap, 1 if retire else 0,
                                         dt if predict else 0.0, None)
            assert rc == 0, product.last_error()
        product.gather_push_ws(C.byref(pv), field_triplet(Ed), field_triplet(Bd), C.byref(g), q, m, dt, order, 1,
                               _capi.PUSHER_BORIS, 1, ws, None)
        if mode:
            rc = product.push_sort_end(ws, 1 if n_retired_in_record else 0, C.byref(live_i64), C.byref(app_i64), None)
            assert rc == 0, product.last_error()
        _sync(product)
        if mode & _capi.PUSH_SORT_SCATTER:
            live, appended = live_i64.value, app_i64.value
            assert live == n_counted - n_retired_in_record and appended == npart - n_counted
            got, got_ids = host_copy(spare, live + appended)
            # every surviving particle arrived with its own pushed data; the retired ones of the record are gone, the
            # ones retired since (id -1 as well) were kept where they had been counted
            retired_of_record = (before_ids == -1) if n_retired_in_record else np.zeros(npart, bool)
            assert retired_of_record.sum() == n_retired_in_record
            keep = ~retired_of_record
            assert keep.sum() == live + appended
            lw, lg = (before_ids != -1) & keep, got_ids != -1
            assert lw.sum() == lg.sum() and (keep & (before_ids == -1)).sum() == (got_ids == -1).sum()
            ow, og = np.argsort(before_ids[lw]), np.argsort(got_ids[lg])
            assert np.array_equal(before_ids[lw][ow], got_ids[lg][og])
            for row in range(7):
                assert H.max_rel_err(got[row][lg][og], want[row][lw][ow]) < 1e-12, row
            assert np.all(got[3][got_ids == -1] == 0.0)
            # the cell-sorted part: keys of the positions before this push (= after the previous one), non-decreasing
            id_to_key = dict(zip(key_ids.tolist(), key_of.tolist()))
            keys = np.array([id_to_key[i] for i in got_ids[:live].tolist() if i != -1])
            assert np.all(np.diff(keys) >= 0)
            # ... and the arrivals behind it in their order
            assert np.array_equal(got_ids[live:], before_ids[n_counted:])
            cur, spare = spare, cur
            npart = live + appended
        else:
            got, got_ids = host_copy(cur, npart)
            assert np.array_equal(got_ids, before_ids)
            for row in range(7):
                assert H.max_rel_err(got[row], want[row]) < 1e-12, row
        if mode & _capi.PUSH_SORT_COUNT:   # what the record should hold: keys of the positions this push produced
            after, after_ids = host_copy(cur, npart)
            where = after[:3]
            if predict:
                gam = np.sqrt(1.0 + (after[4] ** 2 + after[5] ** 2 + after[6] ** 2) / plasma.C_LIGHT ** 2)
                where = [after[d] + after[4 + d] / gam * dt for d in range(3)]
            key_of = _tile_major_key(where, ncell, dx, wrap_flags)
            key_ids = after_ids
            n_counted = npart
            n_retired_in_record = int((after_ids == -1).sum())
        keep_inside(cur, npart)
        if step == 0:
            if retire:   # Redistribute retires a few (after the COUNT: they stay where they were counted) ...
                gone = torch.from_numpy(rng.random(npart) < 0.01).to(DEV)
                cur.idcpu[:npart][gone] = -1
                cur.data[3][:npart][gone] = 0.0
            # ... and appends arrivals
            arr = H.random_particles(n_arrive, ncell, 900, u_scale=30.0)
            for r in range(7):
                cur.data[r][npart:npart + n_arrive] = torch.from_numpy(np.asarray(arr[r])).to(DEV)
            cur.idcpu[npart:npart + n_arrive] = torch.from_numpy(np.arange(10 ** 6, 10 ** 6 + n_arrive, dtype=np.int64)).to(DEV)
            npart += n_arrive
    product.workspace_destroy(ws)


@pytest.mark.skipif(H.HIP_ON_CPU, reason="wraps a device pointer in a torch CUDA tensor")
def test_device_pointer_wrapping(product):
    """The torch.distributed transport wraps raw device pointers handed out by the C++ host layer
    (warpx_amd/distributed.py::_as_tensor); check the view aliases the memory."""
    import torch
    from warpx_amd.distributed import _as_tensor
    f = FieldArray(NCELL, STAG["Ex"], (2, 2, 2), DEV)
    nbytes = 8 * 16
    t = _as_tensor(f.view.p, nbytes, True)
    assert t.is_cuda and t.numel() == nbytes
    t.view(torch.float64).fill_(3.5)
    torch.cuda.synchronize()
    assert np.all(f.storage[f.front:f.front + 16].cpu().numpy() == 3.5)
    u = _as_tensor(f.view.p + 8 * 16, nbytes, True)
    u.copy_(t)
    torch.cuda.synchronize()
    assert np.all(f.storage[f.front + 16:f.front + 32].cpu().numpy() == 3.5)


@pytest.mark.parametrize("ncell", [(24, 20, 16), (25, 9, 7), (130, 6, 5), (300, 8, 8)])
def test_evolve_stencil_configurations_bit_exact(oracle, product, ncell):
    """The EvolveB / EvolveE kernels on odd, even and multi-tile row lengths, bit for bit against the oracle."""
    _two_point_body(oracle, product, ncell)


def _two_point_body(oracle, product, ncell):
    ng = 2
    E = H.random_fields(("Ex", "Ey", "Ez"), ncell, ng, 101)
    B = H.random_fields(("Bx", "By", "Bz"), ncell, ng, 102, scale=1e-8)
    J = H.random_fields(("jx", "jy", "jz"), ncell, 3, 103, scale=1e3)
    Ed, Bd, Jd = (H.clone_fields(x, DEV, True) for x in (E, B, J))
    dx = H.LX / np.asarray(ncell, dtype=np.float64)
    dt = H.yee_dt(dx)
    dinv = H.d3(1.0 / dx)
    for _ in range(2):
        oracle.evolve_b(field_triplet(E), field_triplet(B), 0.5 * dt, dinv, None)
        product.evolve_b(field_triplet(Ed), field_triplet(Bd), 0.5 * dt, dinv, None)
        oracle.evolve_e(field_triplet(E), field_triplet(B), field_triplet(J), dt, dinv, None)
        product.evolve_e(field_triplet(Ed), field_triplet(Bd), field_triplet(Jd), dt, dinv, None)
    _sync(product)
    for a, b in zip(Ed + Bd, E + B):
        assert np.array_equal(a.to_numpy(), b.to_numpy())


RETIRED = 0xFFFFFFFFFFFFFFFF


def _view_n(pa, n):
    """The first n particles of a ParticleArrays as a view."""
    v = pa.view
    v.np = n
    return v


def test_redistribute_ops(oracle, product):
    """wxa_wrap_and_classify / wxa_pack_leavers / retired particles in the sort against the CPU
    restatement: same leaver sets per list, same wrapped positions, same messages, same retirement."""
    import torch
    ncell = (24, 20, 16)
    n = 50000
    rng = np.random.default_rng(77)
    dx = H.LX / np.asarray(ncell)
    plo, phi = np.full(3, -H.LX / 2), np.full(3, H.LX / 2)
    blo = np.array([plo[0], plo[1], plo[2]])
    bhi = np.array([0.0, phi[1], 0.0])          # the brick: lower half in x and z, all of y
    # positions around the brick, up to one cell outside it (and outside the domain on the low side)
    pos = [blo[d] - dx[d] + (bhi[d] - blo[d] + 2 * dx[d]) * rng.random(n) for d in range(3)]
    parts = pos + [1e9 * (0.5 + rng.random(n))] + [1e6 * rng.standard_normal(n) for _ in range(3)]
    ids = np.arange(1, n + 1, dtype=np.uint64)
    ids[rng.random(n) < 0.02] = RETIRED         # retired earlier: never listed again
    pc = ParticleArrays.from_numpy(parts, "cpu", ids.copy())
    pd = ParticleArrays.from_numpy(parts, DEV, ids.view(np.int64))
    periodic, split = H.i3((1, 1, 1)), H.i3((1, 0, 1))
    cap = n
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    lists_d = torch.zeros(6 * cap, dtype=torch.int32, device=DEV)
    lists_c = np.zeros(6 * cap, dtype=np.int32)
    cnt_d, cnt_c = (C.c_int64 * 6)(), (C.c_int64 * 6)()
    product.wrap_and_classify(C.byref(pd.view), 0, n, H.d3(plo), H.d3(phi), periodic, H.d3(blo), H.d3(bhi), split,
                              lists_d.data_ptr(), cap, cnt_d, ws, None)
    oracle.wrap_and_classify(C.byref(pc.view), 0, n, H.d3(plo), H.d3(phi), periodic, H.d3(blo), H.d3(bhi), split,
                             lists_c.ctypes.data, cap, cnt_c, None, None)
    assert list(cnt_d) == list(cnt_c)
    assert cnt_d[2] == 0 and cnt_d[3] == 0 and sum(cnt_d) > 1000       # y is not split
    # the same scan with the leavers listed by destination brick (27 lists), on fresh copies
    pc27 = ParticleArrays.from_numpy(parts, "cpu", ids.copy())
    pd27 = ParticleArrays.from_numpy(parts, DEV, ids.view(np.int64))
    l27_d = torch.zeros(27 * cap, dtype=torch.int32, device=DEV)
    l27_c = np.zeros(27 * cap, dtype=np.int32)
    c27_d, c27_c = (C.c_int64 * 27)(), (C.c_int64 * 27)()
    product.wrap_and_classify_dest(C.byref(pd27.view), 0, n, H.d3(plo), H.d3(phi), periodic, H.d3(blo), H.d3(bhi), split,
                                   l27_d.data_ptr(), cap, c27_d, ws, None)
    oracle.wrap_and_classify_dest(C.byref(pc27.view), 0, n, H.d3(plo), H.d3(phi), periodic, H.d3(blo), H.d3(bhi), split,
                                  l27_c.ctypes.data, cap, c27_c, None, None)
    assert list(c27_d) == list(c27_c) and sum(c27_d) == sum(cnt_d) and c27_d[13] == 0
    l27 = l27_d.cpu().numpy()
    for c in range(27):
        assert np.array_equal(np.sort(l27[c * cap:c * cap + c27_d[c]]), np.sort(l27_c[c * cap:c * cap + c27_c[c]]))
    assert np.array_equal(pd27.to_numpy(), pc27.to_numpy())
    ld = lists_d.cpu().numpy()
    for c in range(6):
        assert np.array_equal(np.sort(ld[c * cap:c * cap + cnt_d[c]]), np.sort(lists_c[c * cap:c * cap + cnt_c[c]]))
    assert np.array_equal(pd.to_numpy(), pc.to_numpy())                 # wrapped positions, bit for bit
    # particles retired earlier are still pushed until the next sort: one that the push carried over a face of the
    # brick is parked inside again instead of being wrapped a whole domain away (its stencils must stay in reach)
    a = pd.to_numpy()
    was_retired = ids == RETIRED
    outside = np.zeros(n, dtype=bool)
    for d in (0, 2):
        outside |= (np.asarray(parts[d]) < blo[d]) | (np.asarray(parts[d]) >= bhi[d])
    assert (was_retired & outside).sum() > 50
    for d in (0, 2):
        assert np.all(a[d, was_retired] >= blo[d]) and np.all(a[d, was_retired] < bhi[d])
    # pack + retire list 1 (towards +x), in the product's list order on both sides
    m = int(cnt_d[1])
    lst = np.ascontiguousarray(ld[cap:cap + m])
    row_len, off = m + 7, 5
    msg_d = torch.zeros(8 * row_len, dtype=torch.float64, device=DEV)
    msg_c = np.zeros(8 * row_len, dtype=np.float64)
    product.pack_leavers(C.byref(pd.view), lists_d.data_ptr() + 4 * cap, m, msg_d.data_ptr(), row_len, off, 1,
                         H.d3(blo), H.d3(bhi), None)
    oracle.pack_leavers(C.byref(pc.view), lst.ctypes.data, m, msg_c.ctypes.data, row_len, off, 1, H.d3(blo),
                        H.d3(bhi), None)
    _sync(product)
    assert np.array_equal(msg_d.cpu().numpy().view(np.uint64), msg_c.view(np.uint64))
    assert np.array_equal(pd.to_numpy(), pc.to_numpy())
    ids_d = pd.idcpu.cpu().numpy().view(np.uint64)
    assert np.array_equal(ids_d, pc.idcpu)
    assert int((ids_d == RETIRED).sum()) == int((ids == RETIRED).sum()) + m
    a = pd.to_numpy()
    assert np.all(a[3, lst] == 0.0) and np.all(a[4:7, lst] == 0.0)
    for d in range(3):
        assert np.all(a[d, lst] >= blo[d]) and np.all(a[d, lst] < bhi[d])
    # the sort drops the retired particles behind the live ones
    out = ParticleArrays(n, DEV, with_id=True)
    bn = (12, 20, 8)
    product.sort_particles_by_cell(C.byref(pd.view), C.byref(out.view), H.d3(blo), H.d3(1.0 / dx), H.i3((0, 0, 0)),
                                   (C.c_int32 * 3)(*bn), ws, None)
    live = C.c_int64()
    product.sort_live_count(ws, C.byref(live), None)
    nlive = int((ids_d != RETIRED).sum())
    assert live.value == nlive
    oid = out.idcpu.cpu().numpy().view(np.uint64)
    assert np.all(oid[:nlive] != RETIRED) and np.all(oid[nlive:] == RETIRED)
    assert np.array_equal(np.sort(oid[:nlive]), np.sort(ids_d[ids_d != RETIRED]))
    product.workspace_destroy(ws)


@pytest.mark.parametrize("order", [1, 3])
def test_tile_kernels_with_appended_tail(oracle, product, order):
    """Arrivals appended behind the sorted part of a tile (Redistribute between two sorts): the
    LDS-tile kernels cover the sorted part, the global-memory kernels the tail; together they must
    equal the CPU result over all particles."""
    import torch
    ncell = (24, 20, 16)
    nsorted, ntail = 30000, 700
    ng_eb, ng_depos, ng_j = H.guard_depths(order, use_filter=True)
    dx = H.LX / np.asarray(ncell)
    head = H.random_particles(nsorted, ncell, 301, u_scale=0.3)
    tail = H.random_particles(ntail, ncell, 302, u_scale=0.3)
    src = ParticleArrays.from_numpy(head, DEV)
    allp = ParticleArrays(nsorted + ntail, DEV)
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    v_sorted = _view_n(allp, nsorted)
    product.sort_particles_by_cell(C.byref(src.view), C.byref(v_sorted), H.d3((-H.LX / 2,) * 3), H.d3(1.0 / dx),
                                   H.i3((0, 0, 0)), (C.c_int32 * 3)(*ncell), ws, None)
    _sync(product)
    allp.data[:, nsorted:] = torch.from_numpy(np.stack(tail)).to(DEV)
    ph = ParticleArrays.from_numpy(list(allp.to_numpy()), "cpu")
    # deposition
    J = [FieldArray(ncell, STAG[n], (ng_j,) * 3, "cpu") for n in ("jx", "jy", "jz")]
    Jd = H.clone_fields(J, DEV, True)
    g, _ = H.geom_for(ncell, ng_depos)
    dt = H.yee_dt(dx)
    q = -plasma.Q_E
    oracle.deposit_current(C.byref(ph.view), field_triplet(J), C.byref(g), q, dt, -0.5 * dt, order, 0, None, None)
    product.deposit_current(C.byref(allp.view), field_triplet(Jd), C.byref(g), q, dt, -0.5 * dt, order, 0, ws, None)
    _sync(product)
    for a, b in zip(Jd, J):
        assert H.max_rel_err(a.to_numpy(), b.to_numpy()) < 1e-12
    # gather + push
    E = H.random_fields(("Ex", "Ey", "Ez"), ncell, ng_eb, 11, 1e9)
    B = H.random_fields(("Bx", "By", "Bz"), ncell, ng_eb, 12, 1.0)
    Ed, Bd = H.clone_fields(E, DEV, True), H.clone_fields(B, DEV, True)
    ge, _ = H.geom_for(ncell, ng_eb)
    oracle.gather_push(C.byref(ph.view), field_triplet(E), field_triplet(B), C.byref(ge), q, plasma.M_E, dt, order, 1,
                       0, None)
    product.gather_push_ws(C.byref(allp.view), field_triplet(Ed), field_triplet(Bd), C.byref(ge), q, plasma.M_E, dt,
                           order, 1, 0, 1, ws, None)
    _sync(product)
    a, b = allp.to_numpy(), ph.to_numpy()
    for r in range(7):
        assert H.max_rel_err(a[r], b[r]) < 1e-13
    product.workspace_destroy(ws)


@pytest.mark.parametrize("pec", [((0, 0, 1), (0, 0, 1)), ((1, 0, 1), (1, 0, 1)), ((0, 1, 0), (0, 0, 0))])
@pytest.mark.parametrize("ng", [0, 1, 2])
def test_apply_pec_fields(oracle, product, pec, ng):
    """wxa_apply_pec_e / wxa_apply_pec_b (PEC::ApplyPECtoEfield / ApplyPECtoBfield) on random fields, one, two
    and one-sided PEC directions, guard depths 0..2: bit-identical to the CPU restatement, guards included."""
    ncell = (12, 10, 14)
    ngalloc = 2
    dom_lo, dom_hi = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*[n - 1 for n in ncell])
    plo, phi = (C.c_int32 * 3)(*pec[0]), (C.c_int32 * 3)(*pec[1])
    g3 = (C.c_int32 * 3)(ng, ng, ng)
    for names, fn in ((("Ex", "Ey", "Ez"), "apply_pec_e"), (("Bx", "By", "Bz"), "apply_pec_b")):
        F = H.random_fields(names, ncell, ngalloc, 7)
        Fd = H.clone_fields(F, DEV, True)
        getattr(oracle, fn)(field_triplet(F), dom_lo, dom_hi, plo, phi, g3, None)
        getattr(product, fn)(field_triplet(Fd), dom_lo, dom_hi, plo, phi, g3, None)
        _sync(product)
        for a, b in zip(Fd, F):
            assert np.array_equal(a.to_numpy(), b.to_numpy())


@pytest.mark.parametrize("pec", [((1, 0, 0), (1, 0, 0)), ((0, 1, 1), (0, 1, 1)), ((0, 0, 1), (0, 0, 0))])
def test_apply_pec_j(oracle, product, pec):
    """wxa_apply_pec_j (PEC::ApplyReflectiveBoundarytoJfield, absorbing particle boundaries) on random J with
    one, two and one-sided PEC directions: bit-identical to the CPU restatement, guards included."""
    ncell = (12, 10, 14)
    dom_lo, dom_hi = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*[n - 1 for n in ncell])
    plo, phi = (C.c_int32 * 3)(*pec[0]), (C.c_int32 * 3)(*pec[1])
    J = H.random_fields(("jx", "jy", "jz"), ncell, 4, 9)
    Jd = H.clone_fields(J, DEV, True)
    oracle.apply_pec_j(field_triplet(J), dom_lo, dom_hi, plo, phi, None)
    product.apply_pec_j(field_triplet(Jd), dom_lo, dom_hi, plo, phi, None)
    _sync(product)
    for a, b in zip(Jd, J):
        assert np.array_equal(a.to_numpy(), b.to_numpy())


UNVERIFIED = H.FIRST_GPU_RUN   # see tests/helpers.py


@UNVERIFIED
def test_apply_particle_boundaries(oracle, product):
    """wxa_apply_particle_boundaries (WarpXParticleContainer::ApplyBoundaryConditions): reflecting x, absorbing
    y, periodic (untouched) z walls on particles scattered around the domain: same survivors, positions,
    momenta and retired marks as the CPU restatement, bit for bit."""
    n = 20000
    rng = np.random.default_rng(3)
    lo, hi = np.full(3, -1.0), np.full(3, 1.0)
    pos = [lo[d] - 0.1 + 2.2 * rng.random(n) for d in range(3)]
    parts = pos + [1.0 + rng.random(n)] + [1e7 * rng.standard_normal(n) for _ in range(3)]
    ids = np.arange(1, n + 1, dtype=np.uint64)
    ids[rng.random(n) < 0.02] = RETIRED
    pc = ParticleArrays.from_numpy(parts, "cpu", ids.copy())
    pd = ParticleArrays.from_numpy(parts, DEV, ids.view(np.int64))
    bc_lo = (C.c_int32 * 3)(_capi.PBOUNDARY_REFLECTING, _capi.PBOUNDARY_ABSORBING, _capi.PBOUNDARY_PERIODIC)
    bc_hi = (C.c_int32 * 3)(_capi.PBOUNDARY_REFLECTING, _capi.PBOUNDARY_ABSORBING, _capi.PBOUNDARY_PERIODIC)
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    lost_c, lost_d = C.c_int64(), C.c_int64()
    oracle.apply_particle_boundaries(C.byref(pc.view), H.d3(lo), H.d3(hi), bc_lo, bc_hi, C.byref(lost_c), None, None)
    product.apply_particle_boundaries(C.byref(pd.view), H.d3(lo), H.d3(hi), bc_lo, bc_hi, C.byref(lost_d), ws, None)
    _sync(product)
    assert lost_c.value == lost_d.value > 100
    assert np.array_equal(pd.to_numpy(), pc.to_numpy())
    assert np.array_equal(pd.idcpu.cpu().numpy().view(np.uint64), pc.idcpu)
    product.workspace_destroy(ws)


@UNVERIFIED
@pytest.mark.parametrize("direction,num_shift", [(2, 1), (2, 2), (0, 1), (1, 3)])
def test_shift_field_window(oracle, product, direction, num_shift):
    """wxa_shift_field_window (WarpX::shiftMF, zero external field): every staggering, window along each axis,
    the other two periodic, shifts of 1..3 cells on padded device rows: bit-identical to the CPU restatement,
    guards included."""
    import torch
    ncell = (12, 10, 14)
    periodic = [1, 1, 1]
    periodic[direction] = 0
    names = ("Ex", "Ey", "Ez", "Bx", "By", "Bz")
    F = H.random_fields(names, ncell, 4, 21)
    Fd = H.clone_fields(F, DEV, True)
    for f, fd in zip(F, Fd):
        tmp_c = np.zeros(f.view.kstride * f.view.n[2])
        tmp_d = torch.zeros(fd.view.kstride * fd.view.n[2], dtype=torch.float64, device=DEV)
        rc = oracle.shift_field_window(C.byref(f.view), tmp_c.ctypes.data, direction, num_shift, H.i3(periodic), None)
        assert rc == 0
        product.shift_field_window(C.byref(fd.view), tmp_d.data_ptr(), direction, num_shift, H.i3(periodic), None)
        _sync(product)
        assert np.array_equal(fd.to_numpy(), f.to_numpy())


@pytest.mark.parametrize("gamma_boost", [1.0, 5.0])
def test_laser_push(oracle, product, gamma_boost):
    """wxa_laser_push (LaserParticleContainer::Evolve: plane coordinates, Gaussian profile with a focal distance,
    update_laser_particle) on an antenna plane of +/- weighted macro-particles at three times around the peak:
    positions and momenta within 1e-13 of the CPU restatement (device exp/sin/cos differ from libm by ulps).
    gamma_boost > 1: the antenna of a boosted frame drifts with -beta c along its normal on top of that."""
    n = 30000
    rng = np.random.default_rng(11)
    par = _capi.LaserPushParams()
    for d, v in enumerate((0.0, 0.0, 9e-6)):
        par.position[d] = v
    for d, v in enumerate((0.0, 1.0, 0.0)):
        par.p_X[d] = v
    for d, v in enumerate((-1.0, 0.0, 0.0)):
        par.p_Y[d] = v
    par.e_max, par.wavelength, par.waist = 16e12, 0.8e-6, 5e-6
    par.duration, par.t_peak, par.focal_distance = 15e-15, 30e-15, 100e-6
    par.mobility = 4e-14                       # |v/c| <= 0.64
    par.gamma_boost = gamma_boost
    for d, v in enumerate((0.0, 0.0, 1.0)):
        par.nvec[d] = v
    x, y = (rng.random(n) - 0.5) * 30e-6, (rng.random(n) - 0.5) * 30e-6
    w = np.where(rng.random(n) < 0.5, 1.0, -1.0) * 1e5
    parts = [x, y, np.full(n, 9e-6), w, np.zeros(n), np.zeros(n), np.zeros(n)]
    dt = 1.3e-16
    for t in (10e-15, 30.2e-15, 47e-15):
        pc = ParticleArrays.from_numpy(parts, "cpu")
        pd = ParticleArrays.from_numpy(parts, DEV)
        assert oracle.laser_push(C.byref(pc.view), C.byref(par), t, dt, None) == 0
        product.laser_push(C.byref(pd.view), C.byref(par), t, dt, None)
        _sync(product)
        a, b = pd.to_numpy(), pc.to_numpy()
        assert np.max(np.abs(b[5])) > 0            # the antenna moves along the polarisation
        if gamma_boost > 1.0:                      # ... and backwards along its normal, all of it alike
            beta = math.sqrt(1.0 - 1.0 / gamma_boost ** 2)
            assert np.allclose(b[2] - 9e-6, -beta * plasma.C_LIGHT * dt, rtol=1e-9)
            assert np.all(b[6] < 0)
        else:
            assert np.all(b[2] == 9e-6) and np.all(b[6] == 0)
        for row in range(7):
            scale = max(np.max(np.abs(b[row])), 1e-300)
            assert np.max(np.abs(a[row] - b[row])) <= 1e-13 * scale, (t, row)


@UNVERIFIED
@pytest.mark.parametrize("pec", [((1, 0, 0), (1, 0, 0)), ((0, 1, 1), (0, 1, 1)), ((0, 0, 1), (0, 0, 0))])
def test_apply_pec_rho(oracle, product, pec):
    """wxa_apply_pec_rho (PEC::ApplyReflectiveBoundarytoRhofield): the J kernel with the sign of a component
    tangential to every wall, on a random nodal rho: bit-identical to the CPU restatement, guards included."""
    ncell = (12, 10, 14)
    dom_lo, dom_hi = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*[n - 1 for n in ncell])
    plo, phi = (C.c_int32 * 3)(*pec[0]), (C.c_int32 * 3)(*pec[1])
    (rho,) = H.random_fields(("rho",), ncell, 5, 13)
    (rho_d,) = H.clone_fields([rho], DEV, True)
    oracle.apply_pec_rho(C.byref(rho.view), dom_lo, dom_hi, plo, phi, None)
    product.apply_pec_rho(C.byref(rho_d.view), dom_lo, dom_hi, plo, phi, None)
    _sync(product)
    assert np.array_equal(rho_d.to_numpy(), rho.to_numpy())


@UNVERIFIED
@pytest.mark.parametrize("grow", [(1, 1, 1), (0, 0, 1), (1, 0, 0)])
def test_evolve_b_guard_layer(oracle, product, grow):
    """wxa_evolve_b_guard_layer after wxa_evolve_b: every point of B, guards included, bit for bit what the CPU
    restatement gives; the valid points are untouched and the face guard layers of the components that are
    cell-centred along a grown direction did change."""
    ncell = (40, 12, 14)
    dinv, dt = H.d3((1e6, 2e6, 3e6)), 1e-15
    g3 = (C.c_int32 * 3)(*grow)
    E = H.random_fields(("Ex", "Ey", "Ez"), ncell, 2, 1)
    B = H.random_fields(("Bx", "By", "Bz"), ncell, 2, 2)
    Ed, Bd = H.clone_fields(E, DEV, True), H.clone_fields(B, DEV, True)
    oracle.evolve_b(field_triplet(E), field_triplet(B), dt, dinv, None)
    before = [b.to_numpy().copy() for b in B]
    oracle.evolve_b_guard_layer(field_triplet(E), field_triplet(B), dt, dinv, g3, None)
    product.evolve_b(field_triplet(Ed), field_triplet(Bd), dt, dinv, None)
    product.evolve_b_guard_layer(field_triplet(Ed), field_triplet(Bd), dt, dinv, g3, None)
    _sync(product)
    for a, b, b0 in zip(Bd, B, before):
        assert np.array_equal(a.to_numpy(), b.to_numpy())
        assert np.array_equal(b.to_numpy()[2:-2, 2:-2, 2:-2], b0[2:-2, 2:-2, 2:-2])
        touched = any(g and not st for g, st in zip(grow, b.stag))
        assert np.array_equal(b.to_numpy(), b0) != touched


@UNVERIFIED
@pytest.mark.parametrize("order,pusher", [(3, _capi.PUSHER_BORIS), (1, _capi.PUSHER_VAY)])
def test_gather_push_in_two_parts(product, order, pusher):
    """wxa_gather_push_part: the interior tiles, then the rest (face tiles + the particles appended since the sort),
    give every particle bit for bit what one wxa_gather_push_ws call gives; the interior part alone moves a
    share of the particles and none that sits in a face tile."""
    import torch
    ncell = (40, 32, 24)   # 5 x 4 x 3 tiles: 6 of them touch no face
    ng, _, _ = H.guard_depths(order)
    E = H.random_fields(("Ex", "Ey", "Ez"), ncell, ng, 10, scale=1e11, device=DEV, pad=True)
    B = H.random_fields(("Bx", "By", "Bz"), ncell, ng, 11, scale=1e3, device=DEV, pad=True)
    parts = H.random_particles(40000, ncell, 77)
    dx = H.LX / np.asarray(ncell)
    pd0 = ParticleArrays.from_numpy(parts, DEV)
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    ntail = 500
    full = ParticleArrays(pd0.np + ntail, DEV)        # room for a tail behind the sorted part
    srt_view = _capi.ParticleView.from_buffer_copy(full.view)
    srt_view.np = pd0.np
    product.sort_particles_by_cell(C.byref(pd0.view), C.byref(srt_view), H.d3((-H.LX / 2,) * 3), H.d3(1.0 / dx),
                                   (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*ncell), ws, None)
    _sync(product)
    full.data[:, pd0.np:] = pd0.data[:, :ntail]       # arrivals since the sort: anywhere in the box
    start = full.data.clone()
    g, _ = H.geom_for(ncell, ng)
    dt = H.yee_dt(dx)
    q, m = -plasma.Q_E, plasma.M_E
    product.gather_push_ws(C.byref(full.view), field_triplet(E), field_triplet(B), C.byref(g), q, m, dt, order, 1,
                           pusher, 1, ws, None)
    _sync(product)
    whole = full.data.clone()
    full.data.copy_(start)
    product.gather_push_part(C.byref(full.view), field_triplet(E), field_triplet(B), C.byref(g), q, m, dt, order, 1,
                             pusher, ws, _capi.PART_INTERIOR, None)
    _sync(product)
    moved = (full.data[0] != start[0]).cpu().numpy()
    assert 0 < moved.sum() < pd0.np and not moved[pd0.np:].any()
    cell = np.floor((start[:3].cpu().numpy() + H.LX / 2) / dx[:, None]).astype(int)
    face = np.zeros(full.np, dtype=bool)
    for d in range(3):
        nt = (ncell[d] + 7) // 8
        face |= (cell[d] // 8 == 0) | (cell[d] // 8 == nt - 1)
    assert not (moved & face).any() and moved[:pd0.np][~face[:pd0.np]].all()
    product.gather_push_part(C.byref(full.view), field_triplet(E), field_triplet(B), C.byref(g), q, m, dt, order, 1,
                             pusher, ws, _capi.PART_REST, None)
    _sync(product)
    assert torch.equal(full.data, whole)
    product.workspace_destroy(ws)


@UNVERIFIED
@pytest.mark.parametrize("ppc,u,uth,gamma_boost,t", [
    ((1, 1, 1), None, None, 1.0, 0.0), ((2, 1, 3), (0.1, -0.2, 0.0), None, 1.0, 0.0),
    ((2, 2, 2), (0.0, 0.0, 0.3), (0.01, 0.02, 0.03), 1.0, 0.0),
    # a lab-frame plasma drifting along z, added at t > 0: the bounds are looked up at the ballistically corrected z
    ((2, 1, 3), (0.1, -0.2, 0.5), None, 1.0, 3e-15),
    # boosted frames: at rest in the lab, and drifting + thermal at t > 0
    ((1, 1, 2), None, None, 2.0, 0.0), ((2, 2, 2), (0.0, 0.0, 0.3), (0.01, 0.02, 0.03), 3.0, 2e-15)])
def test_add_plasma(oracle, product, ppc, u, uth, gamma_boost, t):
    """wxa_add_plasma (PhysicalParticleContainer::AddPlasma on the device): injector bounds cutting through cells,
    a brick smaller than the cell box; at rest and with a constant momentum the same particles as the CPU
    restatement bit for bit (as a set: the device does not promise an order), with gaussian momenta the same
    draws to 1e-13 of the spread (device log / sin / cos differ from libm by ulps) and unit variance.  In a boosted
    frame (the branch at PhysicalParticleContainer.cpp:1210-1247) the same lattice points are kept -- the lab-frame
    bounds are tested at z0_lab -- and weight and u_z carry the Lorentz transform."""
    inj = _capi.PlasmaInjector()
    inj.density = 2e23
    inj.gamma_boost = gamma_boost
    inj.t = t
    for d in range(3):
        inj.ppc[d] = ppc[d]
    lo, hi = (-3.3e-6, -1e300, 0.4e-6), (2.1e-6, 1e300, 1e300)
    for d in range(3):
        inj.lo[d], inj.hi[d] = lo[d], hi[d]
    dx = (0.5e-6, 0.4e-6, 0.25e-6)
    corner, ncells = (-4e-6, -2e-6, 0.0), (16, 10, 12)
    brick_lo, brick_hi = (-4e-6, -2e-6, 0.0), (1.5e-6, 2e-6, 3e-6)
    room = 16 * 10 * 12 * ppc[0] * ppc[1] * ppc[2]
    mom = None
    if u is not None:
        mom = _capi.InjectedMomentum()
        for d in range(3):
            mom.u_mean[d] = u[d]
            mom.u_th[d] = uth[d] if uth else 0.0
        mom.seed = 12345
        for d in range(3):
            mom.origin[d] = corner[d]
    pmom = C.byref(mom) if mom is not None else None
    pc, pd = ParticleArrays(room, "cpu", with_id=True), ParticleArrays(room, DEV, with_id=True)
    nc, nd = C.c_int64(), C.c_int64()
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    args = (C.byref(inj), H.d3(corner), (C.c_int32 * 3)(*ncells), H.d3(dx), H.d3(brick_lo), H.d3(brick_hi), pmom)
    oracle.add_plasma(C.byref(pc.view), *args, C.byref(nc), None, None)
    product.add_plasma(C.byref(pd.view), *args, C.byref(nd), ws, None)
    _sync(product)
    assert nc.value == nd.value and 0 < nc.value < room
    a, b = pd.to_numpy()[:, :nd.value], pc.to_numpy()[:, :nc.value]
    a, b = a[:, np.lexsort(a[:3])], b[:, np.lexsort(b[:3])]
    assert np.array_equal(a[:3], b[:3])
    if gamma_boost == 1.0:
        assert np.array_equal(a[3], b[3])
        assert np.all(b[3] == inj.density * dx[0] * dx[1] * dx[2] / (ppc[0] * ppc[1] * ppc[2]))
    else:
        assert np.max(np.abs(a[3] - b[3])) <= 1e-13 * np.max(b[3])
    if t > 0.0 or gamma_boost > 1.0:   # the z bounds act on the lab-frame image of the lattice
        beta = math.sqrt(1.0 - 1.0 / gamma_boost ** 2)
        ub = u if u is not None else (0.0, 0.0, 0.0)
        bz = ub[2] / math.sqrt(1.0 + ub[0] ** 2 + ub[1] ** 2 + ub[2] ** 2)
        z0 = gamma_boost * (b[2] * (1.0 - beta * bz) - plasma.C_LIGHT * t * (bz - beta))
        assert z0.min() >= lo[2] and (b[2].min() < corner[2] + dx[2] or (z0.min() - lo[2]) < gamma_boost * dx[2] * 1.01)
    if uth is None and gamma_boost == 1.0:
        assert np.array_equal(a, b)
    elif uth is None:
        beta = math.sqrt(1.0 - 1.0 / gamma_boost ** 2)
        for d in range(3):
            assert np.max(np.abs(a[4 + d] - b[4 + d])) <= 1e-14 * plasma.C_LIGHT
        if u is None:   # at rest in the lab: u_z = -gamma beta c, density gamma n
            assert np.allclose(b[6], -gamma_boost * beta * plasma.C_LIGHT, rtol=1e-15)
            assert np.allclose(b[3], gamma_boost * inj.density * dx[0] * dx[1] * dx[2] / (ppc[0] * ppc[1] * ppc[2]), rtol=1e-15)
    else:
        for d in range(3):
            assert np.max(np.abs(a[4 + d] - b[4 + d])) <= 1e-13 * uth[d] * plasma.C_LIGHT * 8 * gamma_boost
        if gamma_boost == 1.0:
            for d in range(3):
                z = (b[4 + d] / plasma.C_LIGHT - u[d]) / uth[d]
                assert abs(z.mean()) < 0.05 and abs(z.std() - 1.0) < 0.05
        else:   # invariants of the transform: n / gamma_particle is a Lorentz scalar per particle
            beta = math.sqrt(1.0 - 1.0 / gamma_boost ** 2)
            g_boosted = np.sqrt(1.0 + (b[4] ** 2 + b[5] ** 2 + b[6] ** 2) / plasma.C_LIGHT ** 2)
            uz_lab = gamma_boost * (b[6] / plasma.C_LIGHT + beta * g_boosted)
            g_lab = np.sqrt(1.0 + (b[4] ** 2 + b[5] ** 2) / plasma.C_LIGHT ** 2 + uz_lab ** 2)
            w0 = inj.density * dx[0] * dx[1] * dx[2] / (ppc[0] * ppc[1] * ppc[2])
            assert np.allclose(b[3] / g_boosted, w0 / g_lab, rtol=1e-12)
            zz = (uz_lab - u[2]) / uth[2]
            assert abs(zz.mean()) < 0.05 and abs(zz.std() - 1.0) < 0.05
    small = ParticleArrays(nc.value - 1, DEV, with_id=True)        # too little room is an error, not an overrun
    with pytest.raises(_capi.WxaError):
        product.add_plasma(C.byref(small.view), *args, C.byref(nd), ws, None)
    product.workspace_destroy(ws)


@pytest.mark.parametrize("cells,ncell,ng,plain", [((1.0, 1.0, 1.0), NCELL, 2, 0), ((1.0, 1.5, 0.8), NCELL, 2, 0),
                                                  ((1.0, 1.5, 0.8), NCELL, 2, 1),
                                                  # several tiles along every direction, partial ones at the high ends,
                                                  # and the minimum guard depth: the staged halo reaches past the arrays
                                                  ((1.0, 1.0, 1.0), (70, 13, 21), 1, 0), ((1.1, 0.9, 1.0), (130, 9, 35), 3, 0),
                                                  # further box shapes (the tile shapes of round 4's timing sweep ran on these)
                                                  ((1.0, 1.0, 1.0), (70, 13, 37), 1, -1), ((1.0, 1.0, 1.0), (70, 13, 37), 1, -3),
                                                  ((1.0, 1.0, 1.0), (70, 13, 37), 1, -4), ((1.0, 1.0, 1.0), (70, 21, 37), 1, -5),
                                                  ((1.0, 1.0, 1.0), (70, 13, 37), 1, -6),
                                                  # planes requested two steps ahead (round 4): short, exact and long marches
                                                  ((1.0, 1.0, 1.0), (70, 13, 37), 1, -7), ((1.1, 0.9, 1.0), (70, 13, 16), 2, -7),
                                                  ((1.0, 1.0, 1.0), (70, 13, 2), 1, -7), ((1.0, 1.0, 1.0), (70, 13, 37), 1, -8),
                                                  ((1.0, 1.0, 1.0), (70, 13, 37), 1, -9), ((1.0, 1.0, 1.0), (70, 13, 67), 1, -10)])
def test_evolve_b_ckc_bit_exact(oracle, product, cells, ncell, ng, plain, monkeypatch):
    """wxa_evolve_b_ckc (EvolveBCartesian<CartesianCKCAlgorithm>) and its coefficients against the CPU restatement:
    same operation order, no contraction -> bit-identical, on cubic and on anisotropic cells, short, exact and long
    marches along z, partial tiles at the high ends."""
    NCELL = ncell
    E = H.random_fields(("Ex", "Ey", "Ez"), NCELL, ng, 61)
    B = H.random_fields(("Bx", "By", "Bz"), NCELL, ng, 62, scale=1e-8)
    Ed, Bd = H.clone_fields(E, DEV, True), H.clone_fields(B, DEV, True)
    dx = np.array(cells) * 0.4e-6
    co = [(C.c_double * 5)() for _ in range(3)]
    cp = [(C.c_double * 5)() for _ in range(3)]
    oracle.ckc_stencil_coefficients(H.d3(dx), *co)
    product.ckc_stencil_coefficients(H.d3(dx), *cp)
    assert all(list(a) == list(b) for a, b in zip(co, cp))
    assert oracle.ckc_max_dt(H.d3(dx)) == product.ckc_max_dt(H.d3(dx))
    dt = 0.5 * product.ckc_max_dt(H.d3(dx))
    oracle.evolve_b_ckc(field_triplet(E), field_triplet(B), dt, *co, None)
    product.evolve_b_ckc(field_triplet(Ed), field_triplet(Bd), dt, *cp, None)
    _sync(product)
    for a, b in zip(Bd, B):
        assert np.array_equal(a.to_numpy(), b.to_numpy())
    # one guard point of E is a precondition, not an overrun
    E0 = [FieldArray(NCELL, STAG[n], (0, 0, 0), DEV) for n in ("Ex", "Ey", "Ez")]
    with pytest.raises(_capi.WxaError):
        product.evolve_b_ckc(field_triplet(E0), field_triplet(Bd), dt, *cp, None)


@UNVERIFIED
def test_empty_inputs_are_no_ops(product):
    """np = 0 through every per-particle entry point (a brick in vacuum, a species before injection): status OK,
    nothing launched with an empty grid, fields untouched."""
    import torch
    ncell = (16, 16, 16)
    E = H.clone_fields(H.random_fields(("Ex", "Ey", "Ez"), ncell, 4, 1), DEV, True)
    B = H.clone_fields(H.random_fields(("Bx", "By", "Bz"), ncell, 4, 2), DEV, True)
    J = H.clone_fields(H.random_fields(("jx", "jy", "jz"), ncell, 5, 3), DEV, True)
    (rho,) = H.clone_fields(H.random_fields(("rho",), ncell, 5, 4), DEV, True)
    before = [f.to_numpy() for f in J + [rho]]
    g, dx = H.geom_for(ncell, 4)
    gj, _ = H.geom_for(ncell, 5)
    dt = H.yee_dt(dx)
    room_a, room_b = ParticleArrays(4, DEV, with_id=True), ParticleArrays(4, DEV, with_id=True)
    empty, out = room_a.view, room_b.view
    empty.np = 0
    out.np = 0
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    q, m = -plasma.Q_E, plasma.M_E
    lo, hi = H.d3((-H.LX / 2,) * 3), H.d3((H.LX / 2,) * 3)
    for order in (1, 2, 3):
        for pusher in (_capi.PUSHER_BORIS, _capi.PUSHER_VAY):
            product.gather_push(C.byref(empty), field_triplet(E), field_triplet(B), C.byref(g), q, m, dt, order, 1, pusher, None)
            product.push_p(C.byref(empty), field_triplet(E), field_triplet(B), C.byref(g), q, m, dt, order, 1, pusher, None)
        for algo in (_capi.DEPOSIT_ESIRKEPOV, _capi.DEPOSIT_DIRECT):
            product.deposit_current(C.byref(empty), field_triplet(J), C.byref(gj), q, dt, -0.5 * dt, order, algo, ws, None)
        product.deposit_charge(C.byref(empty), C.byref(rho.view), C.byref(gj), q, order, None)
    product.enforce_periodic(C.byref(empty), lo, hi, H.i3((1, 1, 1)), None)
    product.sort_particles_by_cell(C.byref(empty), C.byref(out), lo, H.d3(1.0 / dx), (C.c_int32 * 3)(0, 0, 0),
                                   (C.c_int32 * 3)(*ncell), ws, None)
    # (an empty sort records nothing: the tile kernels are not selected, the global-memory path sees np = 0)
    product.deposit_current(C.byref(out), field_triplet(J), C.byref(gj), q, dt, -0.5 * dt, 3, _capi.DEPOSIT_ESIRKEPOV, ws, None)
    cnt = (C.c_int64 * 6)()
    lists = torch.zeros(6, dtype=torch.int32, device=DEV)
    product.wrap_and_classify(C.byref(empty), 0, 0, lo, hi, H.i3((1, 1, 1)), lo, H.d3((0.0, H.LX / 2, 0.0)), H.i3((1, 0, 1)),
                              lists.data_ptr(), 1, cnt, ws, None)
    assert list(cnt) == [0] * 6
    n_lost = C.c_int64(-1)
    product.apply_particle_boundaries(C.byref(empty), lo, hi, (C.c_int32 * 3)(1, 0, 0), (C.c_int32 * 3)(1, 0, 0),
                                      C.byref(n_lost), ws, None)
    assert n_lost.value == 0
    _sync(product)
    for f, a in zip(J + [rho], before):
        assert np.array_equal(f.to_numpy(), a)
    product.workspace_destroy(ws)


@pytest.mark.parametrize("order,sort,gamma_boost", [(1, False, 1.0), (3, True, 1.0), (3, True, 2.0), (2, False, 5.0)])
def test_push_through_a_repeated_plasma_lens(oracle, product, order, sort, gamma_boost):
    """particles.*_ext_particle_init_style = repeated_plasma_lens (GetExternalEBField, GetExternalFields.H:137-189) on top
    of the gathered and the constant external fields: lab frame and boosted frames, electric and magnetic lenses,
    particles before the first lens, inside lenses, stepping over a lens shorter than their step, and beyond the last
    one; PushPX and PushP against the CPU restatement, on the global-memory kernel and on the LDS tiles."""
    ng = 4
    E = H.random_fields(("Ex", "Ey", "Ez"), NCELL, ng, 81, scale=1e6)
    B = H.random_fields(("Bx", "By", "Bz"), NCELL, ng, 82, scale=3e-3)
    Ed, Bd = H.clone_fields(E, DEV, True), H.clone_fields(B, DEV, True)
    g, dx = H.geom_for(NCELL, ng)
    dt = H.yee_dt(dx)
    n = 20000
    parts = H.random_particles(n, NCELL, 83, u_scale=2.0, margin=0.5)
    rng = np.random.default_rng(84)
    parts[6] = np.abs(parts[6]) + 0.05 * plasma.C_LIGHT            # the lens assumes vz > 0 in the lab frame
    q, m = plasma.Q_E, plasma.M_E
    # the lattice in units of the box (z spans [-LX/2, LX/2]): five periods cover the box's lab-frame image, lens 1 is
    # shorter than a step of the fast particles, the last period has no lens (i_lens >= n_lenses)
    uz_boost = math.sqrt(gamma_boost ** 2 - 1.0) * plasma.C_LIGHT
    if gamma_boost == 1.0:
        time = 3.7 * dt
        parts[2] = rng.uniform(0.02 * H.LX, 0.45 * H.LX, n)        # lab frame: lenses only act at z > 0
        z_lab_lo, z_lab_hi = 0.0, 0.45 * H.LX
    else:
        time = gamma_boost * H.LX / uz_boost                       # late enough that the whole box is at z_lab > 0
        z_lab_lo = gamma_boost * (-H.LX / 2) + uz_boost * time
        z_lab_hi = gamma_boost * (H.LX / 2) + uz_boost * time
    period = (z_lab_hi - z_lab_lo) / 5.0
    first = math.floor(z_lab_lo / period)
    nl = first + 4
    starts = [0.1 * period] * nl
    lengths = [0.8 * period] * nl
    lengths[first + 1] = 1e-3 * period
    sE = list(rng.uniform(-1, 1, nl) * 1e13)
    sB = list(rng.uniform(-1, 1, nl) * 3e4)
    lens = _capi.RepeatedPlasmaLens.make(period, starts, lengths, sE, sB, gamma_boost, dt)
    ext_e, ext_b = (3e5, -1e6, 5e5), (1e-3, -4e-4, 7e-4)
    ext6 = (C.c_double * 6)(*ext_e, *ext_b)
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    product.workspace_set_external_particle_fields(ws, H.d3(ext_e), H.d3(ext_b))
    product.workspace_set_repeated_plasma_lens(ws, C.byref(lens))
    product.workspace_set_time(ws, time)
    pd = ParticleArrays.from_numpy(parts, DEV, np.arange(1, n + 1, dtype=np.int64))
    if sort:
        srt = ParticleArrays(pd.np, DEV, with_id=True)
        product.sort_particles_by_cell(C.byref(pd.view), C.byref(srt.view), H.d3((-H.LX / 2,) * 3), H.d3(1.0 / dx),
                                       (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*NCELL), ws, None)
        pd = srt
    fn = oracle._dll.orc_gather_push_lens
    fn.restype = C.c_int
    for move in (1, 0):
        before = pd.to_numpy()
        pc = ParticleArrays.from_numpy(list(before), "cpu")
        rc = fn(C.byref(pc.view), field_triplet(E), field_triplet(B), C.byref(g), C.c_double(q), C.c_double(m), C.c_double(dt),
                order, 1, _capi.PUSHER_BORIS, move, ext6, C.byref(lens), C.c_double(time))
        assert rc == 0
        # the same push without the lens: the lens must matter for most particles, or the comparison proves nothing
        pn = ParticleArrays.from_numpy(list(before), "cpu")
        oracle._dll.orc_gather_push_ext.restype = C.c_int
        oracle._dll.orc_gather_push_ext(C.byref(pn.view), field_triplet(E), field_triplet(B), C.byref(g), C.c_double(q),
                                        C.c_double(m), C.c_double(dt), order, 1, _capi.PUSHER_BORIS, move, ext6)
        product.gather_push_ws(C.byref(pd.view), field_triplet(Ed), field_triplet(Bd), C.byref(g), q, m, dt, order, 1,
                               _capi.PUSHER_BORIS, move, ws, None)
        _sync(product)
        a, b, c0 = pd.to_numpy(), pc.to_numpy(), pn.to_numpy()
        touched = np.mean(np.abs(b[4] - c0[4]) > 1e-6 * np.abs(c0[4]))
        assert 0.25 < touched < 0.95, touched
        for row in range(7):
            assert np.max(np.abs(a[row] - b[row])) <= 1e-12 * max(np.max(np.abs(b[row])), 1e-300), (move, row)
    product.workspace_destroy(ws)


@UNVERIFIED
@pytest.mark.parametrize("order,sort,pusher", [(1, False, _capi.PUSHER_HC), (3, True, _capi.PUSHER_HC),
                                               (3, True, _capi.PUSHER_BORIS_RR), (2, False, _capi.PUSHER_BORIS_RR)])
def test_higuera_cary_push_with_external_fields(oracle, product, order, sort, pusher):
    """algo.particle_pusher = higuera (UpdateMomentumHigueraCary) and the radiation-reaction pusher of
    <species>.do_classical_radiation_reaction (UpdateMomentumBorisWithRadiationReaction) with the container's constant external fields
    (particles.E/B_external_particle) on top of the gathered ones: PushPX and PushP against the CPU restatement,
    on the global-memory kernel and on the LDS tiles."""
    ng = 4
    E = H.random_fields(("Ex", "Ey", "Ez"), NCELL, ng, 71, scale=1e10)
    B = H.random_fields(("Bx", "By", "Bz"), NCELL, ng, 72, scale=30.0)
    Ed, Bd = H.clone_fields(E, DEV, True), H.clone_fields(B, DEV, True)
    g, dx = H.geom_for(NCELL, ng)
    dt = H.yee_dt(dx)
    parts = H.random_particles(20000, NCELL, 73, u_scale=2.0, margin=0.5)
    q, m = plasma.Q_E, plasma.M_E
    ext_e, ext_b = (3e9, -1e10, 5e9), (10.0, -4.0, 7.0)
    ext6 = (C.c_double * 6)(*ext_e, *ext_b)
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    product.workspace_set_external_particle_fields(ws, H.d3(ext_e), H.d3(ext_b))
    pd = ParticleArrays.from_numpy(parts, DEV, np.arange(1, 20001, dtype=np.int64))
    if sort:
        srt = ParticleArrays(pd.np, DEV, with_id=True)
        product.sort_particles_by_cell(C.byref(pd.view), C.byref(srt.view), H.d3((-H.LX / 2,) * 3), H.d3(1.0 / dx),
                                       (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*NCELL), ws, None)
        pd = srt
    for move in (1, 0):
        pc = ParticleArrays.from_numpy(list(pd.to_numpy()), "cpu")
        oracle._dll.orc_gather_push_ext.restype = C.c_int
        rc = oracle._dll.orc_gather_push_ext(C.byref(pc.view), field_triplet(E), field_triplet(B), C.byref(g), C.c_double(q),
                                             C.c_double(m), C.c_double(dt), order, 1, pusher, move, ext6)
        assert rc == 0
        product.gather_push_ws(C.byref(pd.view), field_triplet(Ed), field_triplet(Bd), C.byref(g), q, m, dt, order, 1,
                               pusher, move, ws, None)
        _sync(product)
        a, b = pd.to_numpy(), pc.to_numpy()
        for row in range(7):
            assert np.max(np.abs(a[row] - b[row])) <= 1e-12 * max(np.max(np.abs(b[row])), 1e-300), (move, row)
        if move:
            with_ext = b
    # without the workspace the external fields are zero: PushPX of the grid fields alone, and not the result above
    # (the external E alone kicks by 5e-3 of the momentum scale)
    pz = ParticleArrays.from_numpy(parts, DEV)
    product.gather_push(C.byref(pz.view), field_triplet(Ed), field_triplet(Bd), C.byref(g), q, m, dt, order, 1,
                        pusher, None)
    _sync(product)
    po = ParticleArrays.from_numpy(parts, "cpu")
    oracle.gather_push(C.byref(po.view), field_triplet(E), field_triplet(B), C.byref(g), q, m, dt, order, 1, pusher, None)
    a, b = pz.to_numpy(), po.to_numpy()
    unsorted = pd.ids_to_numpy() - 1
    for row in range(7):
        assert np.max(np.abs(a[row] - b[row])) <= 1e-12 * max(np.max(np.abs(b[row])), 1e-300), row
    for row in (4, 5, 6):
        assert np.max(np.abs(a[row][unsorted] - with_ext[row])) > 1e-4 * np.max(np.abs(with_ext[row])), row
    product.workspace_destroy(ws)


@pytest.mark.parametrize("name,box", [("Ex", "owned"), ("Bz", "owned"), ("rho", "valid"), ("jy", "all")])
def test_reduce_field(oracle, product, name, box):
    """wxa_reduce_field (FieldEnergy.cpp:81-157: MultiFab::norm2 / norminf of one component) against the oracle's
    long-double loop and numpy on the same box: the points a brick owns (valid minus the duplicated high node), the
    valid points, the whole allocation.  More points than one pass of 1024 workgroups x 256 lanes covers at once."""
    ncell = (72, 64, 60)
    ng = 3
    f = H.random_fields((name,), ncell, ng, 41, scale=3.0e9)[0]
    fd = f.copy_to(DEV, pad=True)
    v = f.view
    if box == "all":
        lo = [v.lo[d] for d in range(3)]
        hi = [v.lo[d] + v.n[d] for d in range(3)]
    else:
        lo = [v.lo[d] + v.ng[d] for d in range(3)]
        hi = [v.lo[d] + v.n[d] - v.ng[d] - (v.stag[d] if box == "owned" else 0) for d in range(3)]
    assert (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]) > 1024 * 256
    a = f.to_numpy()   # [i][j][k], guards included
    sl = tuple(slice(lo[d] - v.lo[d], hi[d] - v.lo[d]) for d in range(3))
    x = a[sl].astype(np.longdouble)
    ref_s, ref_m = float(np.sum(x * x)), float(np.max(np.abs(a[sl])))
    lo32, hi32 = (C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*hi)
    res = {}
    for lib, arr in ((oracle, f), (product, fd)):
        s, m = C.c_double(), C.c_double()
        lib.reduce_field(C.byref(arr.view), lo32, hi32, C.byref(s), C.byref(m), None)
        res[lib.prefix] = (s.value, m.value)
        assert abs(s.value - ref_s) <= 1e-13 * ref_s, (lib.prefix, s.value, ref_s)
        assert m.value == ref_m, lib.prefix
    # the same input gives the same bits (two passes in a fixed order, no atomics)
    s2 = C.c_double()
    product.reduce_field(C.byref(fd.view), lo32, hi32, C.byref(s2), None, None)
    assert s2.value == res[product.prefix][0]
    # an empty box, and a box that leaves the array
    hi0 = (C.c_int32 * 3)(lo[0], hi[1], hi[2])
    product.reduce_field(C.byref(fd.view), lo32, hi0, C.byref(s2), None, None)
    assert s2.value == 0.0
    bad = (C.c_int32 * 3)(hi[0] + 100, hi[1], hi[2])
    with pytest.raises(_capi.WxaError):
        product.reduce_field(C.byref(fd.view), lo32, bad, C.byref(s2), None, None)


@pytest.mark.parametrize("n,photon", [(300_000, 0), (777, 0), (50_000, 1), (0, 0)])
def test_reduce_particles(oracle, product, n, photon):
    """wxa_reduce_particles (ParticleEnergy.cpp:95-200 with KineticEnergy.H:33-67, ParticleMomentum.cpp:122-253,
    ParticleNumber.cpp:97-139) against the oracle and numpy: sum w Ekin, sum w, sum w m u, number of live particles; a
    tenth of the slots retired (weight and momentum zeroed, idcpu = WXA_IDCPU_RETIRED) as Redistribute leaves them."""
    rng = np.random.default_rng(5)
    parts = H.random_particles(n, NCELL, 77, u_scale=1.5)
    ids = np.zeros(n, dtype=np.uint64)
    retired = rng.random(n) < 0.1
    ids[retired] = np.uint64(0xFFFFFFFFFFFFFFFF)
    for c in (3, 4, 5, 6):
        parts[c] = np.where(retired, 0.0, parts[c])
    m = plasma.M_E * 3.0
    ph = ParticleArrays.from_numpy(parts, "cpu", idcpu=ids)
    pd = ParticleArrays.from_numpy(parts, DEV, idcpu=ids.view(np.int64))
    w, ux, uy, uz = (np.asarray(parts[c], dtype=np.longdouble) for c in (3, 4, 5, 6))
    u2 = ux * ux + uy * uy + uz * uz
    if photon:
        ekin = np.longdouble(plasma.M_E * plasma.C_LIGHT) * np.sqrt(u2)
    else:
        ekin = m * u2 / (1.0 + np.sqrt(1.0 + u2 / np.longdouble(plasma.C_LIGHT) ** 2))
    ref = [float(np.sum(w * ekin)), float(np.sum(w)), float(np.sum(w * m * ux)), float(np.sum(w * m * uy)),
           float(np.sum(w * m * uz)), float(n - np.count_nonzero(retired))]
    scale = [ref[0], ref[1]] + [float(np.sum(w * m * np.abs(c))) for c in (ux, uy, uz)] + [1.0]
    got = {}
    for lib, arr in ((oracle, ph), (product, pd)):
        out = (C.c_double * 6)()
        lib.reduce_particles(C.byref(arr.view), m, photon, out, None)
        got[lib.prefix] = list(out)
        for c in range(6):
            assert abs(out[c] - ref[c]) <= 1e-13 * max(scale[c], 1e-300), (lib.prefix, c, out[c], ref[c])
        assert out[5] == ref[5]
    out2 = (C.c_double * 6)()
    product.reduce_particles(C.byref(pd.view), m, photon, out2, None)
    assert list(out2) == got[product.prefix]
