"""wxa_add_plasma_profile: PhysicalParticleContainer::AddPlasma with the density (and optionally the momenta) given as
expressions that the device evaluates, against the numpy restatement of tests/plasma_profile_model.py.

Geometry of test_add_plasma: 16 x 10 x 12 cells of (0.5, 0.4, 0.25) um, injector bounds that cut through cells, a brick
smaller than the cell box.  The device promises no order: both sets are sorted by position first.

Measured max |dw| over the profile's peak weight, on an MI355X / under the CPU execution model (gate 1e-13): cosine ramp
0 / 0, gaussian x tanh 2.8e-16 / 1.8e-16, parabolic_channel 0 / 0."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import helpers as H
from tests import plasma_profile_model as M
from warpx_amd import _capi
from warpx_amd.containers import ParticleArrays

pytestmark = pytest.mark.gpu

DX = (0.5e-6, 0.4e-6, 0.25e-6)
CORNER, NCELLS = (-4e-6, -2e-6, 0.0), (16, 10, 12)
LO, HI = (-3.3e-6, -1e300, 0.4e-6), (2.1e-6, 1e300, 1e300)
BRICK_LO, BRICK_HI = (-4e-6, -2e-6, 0.0), (1.5e-6, 2e-6, 3e-6)
GEOM = dict(corner=CORNER, ncells=NCELLS, dx=DX, lo=LO, hi=HI, brick_lo=BRICK_LO, brick_hi=BRICK_HI)

N0, ZS, LRAMP, RC2 = 2e23, 0.6e-6, 2e-6, 9e-12
WT, ZC, LT = 2.5e-6, 1.5e-6, 0.5e-6
K = {"n0": N0, "zs": ZS, "L": LRAMP, "rc2": RC2, "w": WT, "zc": ZC, "Lt": LT, "pi": math.pi}

RAMP = "n0*(z-zs)/L*(1+4*(x*x+y*y)/rc2)*(z>=zs)"
COSINE = "n0*0.5*(1-cos(pi*(z-zs)/L))*(z>=zs)*(z<zs+L)+n0*(z>=zs+L)"
GAUSS_TANH = "n0*exp(-(x^2+y^2)/w^2)*0.5*(1+tanh((z-zc)/Lt))"


def ramp(x, y, z):
    return N0 * (z - ZS) / LRAMP * (1 + 4 * (x * x + y * y) / RC2) * (z >= ZS)


def cosine(x, y, z):
    return N0 * 0.5 * (1 - np.cos(math.pi * (z - ZS) / LRAMP)) * (z >= ZS) * (z < ZS + LRAMP) + N0 * (z >= ZS + LRAMP)


def gauss_tanh(x, y, z):
    return N0 * np.exp(-(x * x + y * y) / (WT * WT)) * 0.5 * (1 + np.tanh((z - ZC) / LT))


@pytest.fixture(scope="module")
def ws(product):
    w = C.c_void_p()
    product.workspace_create(C.byref(w))
    yield w
    product.workspace_destroy(w)


def injector(ppc, gamma_boost=1.0, t=0.0, lo=LO, hi=HI):
    inj = _capi.PlasmaInjector()
    inj.density = 0.0
    inj.gamma_boost, inj.t = gamma_boost, t
    for d in range(3):
        inj.ppc[d] = ppc[d]
        inj.lo[d], inj.hi[d] = lo[d], hi[d]
    return inj


def device_add(product, ws, density, ppc, momentum=None, gamma_boost=1.0, t=0.0, density_min=0.0, density_max=M.FLT_MAX,
               geom=GEOM, room=None, raw=False, constant_momentum=None):
    """the particles wxa_add_plasma_profile adds for expression `density` (an _capi.Expr), sorted by position"""
    inj = injector(ppc, gamma_boost, t, geom["lo"], geom["hi"])
    nc = geom["ncells"]
    if room is None:
        room = nc[0] * nc[1] * nc[2] * ppc[0] * ppc[1] * ppc[2]
    pd = ParticleArrays(room, H.DEVICE, with_id=True)
    n = C.c_int64()
    mom = (C.c_void_p * 3)(*[m.handle for m in momentum]) if momentum else None
    call = product._add_plasma_profile if raw else product.add_plasma_profile
    rc = call(C.byref(pd.view), C.byref(inj), H.d3(geom["corner"]), (C.c_int32 * 3)(*nc), H.d3(geom["dx"]),
              H.d3(geom["brick_lo"]), H.d3(geom["brick_hi"]),
              C.byref(constant_momentum) if constant_momentum is not None else None, density.handle, mom, density_min, density_max,
              C.byref(n), ws, None)
    H.device_sync()
    if raw:
        return rc
    got = pd.to_numpy()[:, :n.value]
    assert np.all(pd.ids_to_numpy()[:n.value] == 0)
    return M.sort_by_position(got)


def test_ramp_is_the_models_set_bit_for_bit(product, ws):
    """(a) a linear ramp in z times a transverse parabola, cut off below its foot; ppc (2, 1, 3)"""
    e = _capi.Expr(product, RAMP, constants=K)
    got = device_add(product, ws, e, (2, 1, 3))
    want, _ = M.add_plasma(ramp, ppc=(2, 1, 3), **GEOM)
    assert 0 < want.shape[1] < 16 * 10 * 12 * 6
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.all(got[4:] == 0.0)


@pytest.mark.parametrize("text,fn", [(COSINE, cosine), (GAUSS_TANH, gauss_tanh)], ids=["cosine", "gauss_tanh"])
def test_transcendental_profiles(product, ws, text, fn):
    """(b) same lattice points bit for bit; the weights within 1e-13 of the profile's peak weight (absolute: 1 - cos
    cancels at the foot of the ramp)"""
    e = _capi.Expr(product, text, constants=K)
    got = device_add(product, ws, e, (1, 2, 2))
    want, _ = M.add_plasma(fn, ppc=(1, 2, 2), **GEOM)
    assert want.shape[1] > 1000 and got.shape == want.shape
    assert np.array_equal(got[:3], want[:3])
    worst = np.max(np.abs(got[3] - want[3])) / np.max(want[3])
    print(f"max |dw| / peak weight = {worst:.3e}")
    assert worst <= 1e-13


def test_density_min_drops_the_foot_and_density_max_clips_the_top(product, ws):
    """(c) no lattice point's density lies within 1e-9 (relative) of either threshold, so no rounding decides"""
    dmin, dmax = 0.3 * N0, 0.8 * N0
    e = _capi.Expr(product, RAMP, constants=K)
    got = device_add(product, ws, e, (2, 1, 3), density_min=dmin, density_max=dmax)
    want, raw = M.add_plasma(ramp, ppc=(2, 1, 3), density_min=dmin, density_max=dmax, **GEOM)
    free, free_raw = M.add_plasma(ramp, ppc=(2, 1, 3), **GEOM)
    for thr in (dmin, dmax):
        assert np.min(np.abs(free_raw - thr)) > 1e-9 * thr
    assert (free_raw < dmin).any() and (free_raw > dmax).any()
    assert want.shape[1] == int((free_raw >= dmin).sum()) < free.shape[1]
    wmax = dmax * (DX[0] * DX[1] * DX[2] / 6)
    assert (want[3] == wmax).sum() == int((raw > dmax).sum()) > 0 and want[3].max() == wmax
    assert got.shape == want.shape and np.array_equal(got, want)


def test_a_slab_between_probe_planes_emits_nothing(product, ws):
    """(d) n0 (z > za) (z < zb), ppc_z = 4.  A slab strictly between a cell's low plane and its mid plane holds the
    lattice plane at 3/8 of the cell but none of the 27 probe points: the reference's cell test (:1032-1048) finds no
    density and the cell emits nothing.  A slab over the mid plane is found."""
    dz = DX[2]
    cells = dict(GEOM)
    for za, zb, emits in ((5 * dz + 0.30 * dz, 5 * dz + 0.45 * dz, False), (7 * dz + 0.30 * dz, 7 * dz + 0.70 * dz, True)):
        def slab(x, y, z, za=za, zb=zb):
            return N0 * (z > za) * (z < zb)
        e = _capi.Expr(product, "n0*(z>za)*(z<zb)", constants={"n0": N0, "za": za, "zb": zb})
        got = device_add(product, ws, e, (1, 1, 4), geom=cells)
        want, _ = M.add_plasma(slab, ppc=(1, 1, 4), **cells)
        # the lattice has a plane inside either slab
        zl = np.array([(k + (0.5 + i) / 4) * dz for k in range(12) for i in range(4)])
        assert ((zl > za) & (zl < zb)).any()
        assert got.shape == want.shape and np.array_equal(got, want)
        assert (want.shape[1] > 0) == emits
        if emits:   # the particles of the found cells that sit in the slab carry its density, the others weight 0
            in_slab = (got[2] > za) & (got[2] < zb)
            assert in_slab.any() and np.all(got[3][in_slab] > 0) and np.all(got[3][~in_slab] == 0)


def test_parabolic_channel(product, ws):
    """(e) profile = predefined, parabolic_channel: ramps and plateau a few cells long; gate of (b)"""
    params = (0.5e-6, 0.9e-6, 0.6e-6, 0.8e-6, 4e-6, N0)
    e = _capi.Expr.predefined(product, "parabolic_channel", params)
    got = device_add(product, ws, e, (1, 1, 2))
    want, _ = M.add_plasma(M.parabolic_channel(params), ppc=(1, 1, 2), **GEOM)
    assert want.shape[1] > 500 and got.shape == want.shape
    assert np.array_equal(got[:3], want[:3])
    z = want[2] - params[0]
    for a, b in ((0, params[1]), (params[1], params[1] + params[2]), (params[1] + params[2], sum(params[1:4]))):
        assert ((z > a) & (z < b)).sum() > 50   # every branch of the profile holds lattice points
    worst = np.max(np.abs(got[3] - want[3])) / np.max(want[3])
    print(f"max |dw| / peak weight = {worst:.3e}")
    assert worst <= 1e-13


def test_predefined_refusals(product):
    h = C.c_void_p()
    p6 = (C.c_double * 6)(0, 1, 1, 1, 1, 1)
    assert product._expr_predefined(b"parabolic_channel", p6, 5, C.byref(h)) == -1
    assert "takes 6 values" in product._last_error().decode() and "got 5" in product._last_error().decode()
    assert product._expr_predefined(b"gaussian_blob", p6, 6, C.byref(h)) == -1
    assert "gaussian_blob" in product._last_error().decode()


def test_boosted_frame(product, ws):
    """(f) gamma = 3, t > 0, at rest in the lab: the density is looked up at z0_lab; same lattice points, weights
    gamma n dV / nppc within 1e-13 relative, u_z = -gamma beta c"""
    gamma, t = 3.0, 2e-15
    e = _capi.Expr(product, GAUSS_TANH, constants=K)
    got = device_add(product, ws, e, (2, 2, 2), gamma_boost=gamma, t=t)
    want, _ = M.add_plasma(gauss_tanh, ppc=(2, 2, 2), gamma_boost=gamma, t=t, **GEOM)
    assert want.shape[1] > 1000 and got.shape == want.shape
    assert np.array_equal(got[:3], want[:3])
    assert np.all(np.abs(got[3] - want[3]) <= 1e-13 * want[3])
    assert np.all(got[4:6] == 0.0) and np.max(np.abs(got[6] - want[6])) <= 1e-14 * M.C_LIGHT
    beta = math.sqrt(1 - 1 / gamma ** 2)
    assert np.allclose(want[6], -gamma * beta * M.C_LIGHT, rtol=1e-15)


@pytest.mark.parametrize("gamma,t", [(1.0, 3e-15), (2.0, 3e-16)], ids=["lab", "boosted"])
def test_parsed_momenta(product, ws, gamma, t):
    """(g) ux = 0.1 x / Lx + 0.05 z / Lz, uz = 0.2 + 0.1 y / Ly at t > 0.  Lab frame: the bounds, the density and u are
    taken at the ballistically corrected z (with the bulk momentum at the lattice point).  gamma = 2: u at (x, y, 0).
    The z term of ux (beyond the issue's expressions) is what shows where z is taken: 0.05 (z - z0) / Lz is 1e-3 and
    more, against a gate of 1e-14."""
    lx, ly, lz = 4e-6, 2e-6, 3e-6
    consts = {"Lx": lx, "Ly": ly, "Lz": lz}
    mom = [_capi.Expr(product, s, constants=consts) for s in ("0.1*x/Lx+0.05*z/Lz", "0.0", "0.2+0.1*y/Ly")]
    fns = (lambda x, y, z: 0.1 * x / lx + 0.05 * z / lz, lambda x, y, z: 0.0 * x, lambda x, y, z: 0.2 + 0.1 * y / ly)
    e = _capi.Expr(product, RAMP, constants=K)
    got = device_add(product, ws, e, (2, 1, 3), momentum=mom, gamma_boost=gamma, t=t)
    want, _ = M.add_plasma(ramp, ppc=(2, 1, 3), momentum=fns, gamma_boost=gamma, t=t, **GEOM)
    at_rest, _ = M.add_plasma(ramp, ppc=(2, 1, 3), gamma_boost=gamma, t=t, **GEOM)
    assert want.shape[1] > 1000 and want.shape != at_rest.shape   # the drift moves the z bound across lattice planes
    assert got.shape == want.shape and np.array_equal(got[:3], want[:3])
    if gamma == 1.0:
        assert np.array_equal(got[3], want[3])
    else:
        assert np.all(np.abs(got[3] - want[3]) <= 1e-13 * want[3])
    for d in range(3):
        assert np.max(np.abs(got[4 + d] - want[4 + d])) <= 1e-14 * M.C_LIGHT
    assert np.ptp(want[4]) > 0.05 * M.C_LIGHT and np.ptp(want[6]) > 0.01 * M.C_LIGHT


@pytest.mark.parametrize("ppc,u,uth,gamma_boost,t", [   # the parameter sets of test_kernels_gpu.py::test_add_plasma
    ((1, 1, 1), None, None, 1.0, 0.0), ((2, 1, 3), (0.1, -0.2, 0.0), None, 1.0, 0.0),
    ((2, 2, 2), (0.0, 0.0, 0.3), (0.01, 0.02, 0.03), 1.0, 0.0), ((2, 1, 3), (0.1, -0.2, 0.5), None, 1.0, 3e-15),
    ((1, 1, 2), None, None, 2.0, 0.0), ((2, 2, 2), (0.0, 0.0, 0.3), (0.01, 0.02, 0.03), 3.0, 2e-15)],
    ids=["at_rest", "constant", "gaussian", "drift_t", "gamma2", "gamma3_thermal_t"])
def test_the_constant_entry_and_the_one_operation_profile_agree(product, ws, ppc, u, uth, gamma_boost, t):
    """wxa_add_plasma against wxa_add_plasma_profile with the program "n0", the same wxa_injected_momentum (the profile
    entry's thermal branch), no momentum expressions, no thresholds: the two entries share the lattice decode, the slot
    allocation and the store.  Same lattice points bit for bit; in the lab frame without a thermal spread every column
    bit for bit (weights and momenta are one multiplication each); otherwise the gates of test_add_plasma, since the two
    kernels are separate compilations with contraction allowed in the store.
    Worst deviations measured on an MI355X / under the CPU execution model: 0 / 0 in every column of all six cases."""
    mom = None
    if u is not None:
        mom = _capi.InjectedMomentum()
        for d in range(3):
            mom.u_mean[d], mom.u_th[d], mom.origin[d] = u[d], uth[d] if uth else 0.0, CORNER[d]
        mom.seed = 12345
    inj = injector(ppc, gamma_boost, t)
    inj.density = N0
    room = NCELLS[0] * NCELLS[1] * NCELLS[2] * ppc[0] * ppc[1] * ppc[2]
    pd = ParticleArrays(room, H.DEVICE, with_id=True)
    n = C.c_int64()
    product.add_plasma(C.byref(pd.view), C.byref(inj), H.d3(CORNER), (C.c_int32 * 3)(*NCELLS), H.d3(DX), H.d3(BRICK_LO),
                       H.d3(BRICK_HI), C.byref(mom) if mom is not None else None, C.byref(n), ws, None)
    H.device_sync()
    assert 0 < n.value < room
    a = M.sort_by_position(pd.to_numpy()[:, :n.value])
    b = device_add(product, ws, _capi.Expr(product, "n0", constants={"n0": N0}), ppc, gamma_boost=gamma_boost, t=t,
                   density_min=0.0, density_max=M.FLT_MAX, constant_momentum=mom)
    assert a.shape == b.shape
    assert np.array_equal(a[:3], b[:3])
    dw = np.max(np.abs(a[3] - b[3])) / np.max(a[3])
    du = [np.max(np.abs(a[4 + d] - b[4 + d])) / M.C_LIGHT for d in range(3)]
    print(f"max |dw| / max w = {dw:.3e}, max |du| / c = {du[0]:.3e} {du[1]:.3e} {du[2]:.3e}")
    if gamma_boost == 1.0:
        assert np.array_equal(a[3], b[3])
    if uth is None and gamma_boost == 1.0:
        assert np.array_equal(a, b)
    else:
        assert dw <= 1e-13
        for d in range(3):
            assert du[d] <= (1e-14 if uth is None else 1e-13 * uth[d] * 8 * gamma_boost)


def test_constant_and_parsed_momenta_exclude_each_other(product, ws):
    e = _capi.Expr(product, RAMP, constants=K)
    mom = (C.c_void_p * 3)(e.handle, e.handle, e.handle)
    cm = _capi.InjectedMomentum()
    inj = injector((1, 1, 1))
    pd = ParticleArrays(16 * 10 * 12, H.DEVICE, with_id=True)
    n = C.c_int64()
    rc = product._add_plasma_profile(C.byref(pd.view), C.byref(inj), H.d3(CORNER), (C.c_int32 * 3)(*NCELLS), H.d3(DX),
                                     H.d3(BRICK_LO), H.d3(BRICK_HI), C.byref(cm), e.handle, mom, 0.0, 1e300, C.byref(n), ws, None)
    assert rc == -1 and "both" in product._last_error().decode()


def test_two_bricks_add_what_one_brick_adds(product, ws):
    """(h) two bricks that meet at a cell face in x, each given the whole cell box (as find_overlap's box reaches one cell
    past a brick): the union of the two calls is the one call's set over the joined brick, bit for bit"""
    e = _capi.Expr(product, RAMP, constants=K)
    whole = dict(GEOM, brick_lo=(-4e-6, -2e-6, 0.0), brick_hi=(4e-6, 2e-6, 3e-6))
    one = device_add(product, ws, e, (2, 1, 3), geom=whole)
    xs = CORNER[0] + 7 * DX[0]
    left = dict(whole, brick_hi=(xs, 2e-6, 3e-6))
    right = dict(whole, brick_lo=(xs, -2e-6, 0.0))
    parts = [device_add(product, ws, e, (2, 1, 3), geom=g) for g in (left, right)]
    assert parts[0].shape[1] > 500 and parts[1].shape[1] > 500
    assert np.all(parts[0][0] < xs) and np.all(parts[1][0] > xs)
    assert np.array_equal(M.sort_by_position(np.concatenate(parts, axis=1)), one)
    want, _ = M.add_plasma(ramp, ppc=(2, 1, 3), **whole)
    assert np.array_equal(one, want)


def test_too_little_room_is_an_error(product, ws):
    """(i) room for one particle fewer than needed: WXA_ERR_NOMEM, not an overrun"""
    e = _capi.Expr(product, RAMP, constants=K)
    want, _ = M.add_plasma(ramp, ppc=(2, 1, 3), **GEOM)
    rc = device_add(product, ws, e, (2, 1, 3), room=want.shape[1] - 1, raw=True)
    assert rc == -4   # WXA_ERR_NOMEM
    assert "not enough room" in product._last_error().decode()
    assert device_add(product, ws, e, (2, 1, 3), room=want.shape[1]).shape == want.shape
