"""boundary.field_lo/hi = absorbing_silver_mueller on the HIP path: wxa_apply_silver_mueller and the step that calls it.

The CPU oracle has no Silver-Mueller boundary.  The yardstick is a numpy model written from the reference's formulas
(FiniteDifferenceSolver::ApplySilverMuellerBoundary, 3-D branch, ApplySilverMuellerBoundary.cpp:173-350, around the Yee
update of EvolveB.cpp:164-186 / EvolveE.cpp:177-215), stepped in the reference's schedule: B half, boundary, fill, E,
fill, B half.  Also under WXA_HIP_ON_CPU=1 (tests/hipcpu)."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

from tests import helpers as H
from tests.test_multibrick_gpu import ThreadBrickTransport, thread_transport_abort, thread_transport_state
from warpx_amd import _capi, plasma
from warpx_amd.containers import STAG, FieldArray, field_triplet
from warpx_amd.distributed import brick_coord
from warpx_amd.sim import WarpXSim, field_energy

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DECK = os.path.join(HERE, "decks", "silver_mueller_3d.inputs")
EN, BN = ("Ex", "Ey", "Ez"), ("Bx", "By", "Bz")
CL = plasma.C_LIGHT
P, PEC, S = _capi.BOUNDARY_PERIODIC, _capi.BOUNDARY_PEC, 2   # 2: WXA_BOUNDARY_SILVER_MUELLER (include/warpx_amd.h)


# ---- the numpy model ---------------------------------------------------------------------------------------------------
# Arrays are dense [i, j, k] with guards, as WarpXSim.field() returns them; array index = global index - lo.

# The twelve point rules of :238-346 in the reference's order: component, direction of the face, side, sign in front of
# coef2, the component of E it reads (at the same indices on a hi face, one point further in along the direction on a lo face).
SM_RULES = (
    ("Bx", 1, "hi", +1, "Ez"), ("Bx", 1, "lo", -1, "Ez"), ("Bx", 2, "hi", -1, "Ey"), ("Bx", 2, "lo", +1, "Ey"),
    ("By", 0, "hi", -1, "Ez"), ("By", 0, "lo", +1, "Ez"), ("By", 2, "hi", +1, "Ex"), ("By", 2, "lo", -1, "Ex"),
    ("Bz", 0, "hi", +1, "Ey"), ("Bz", 0, "lo", -1, "Ey"), ("Bz", 1, "hi", -1, "Ex"), ("Bz", 1, "lo", +1, "Ex"),
)


def sm_apply(F, lo, ncell, ng, dt, dinv, dom_lo, dom_hi, sm_lo, sm_hi, tol=None):
    """The boundary on the brick with `ncell` cells whose arrays start at global index `lo`, in place.  tol (a dict of
    arrays of zeros like the components of B): receives the round-off allowance of every updated point, 2^-52 (|coef1 B| +
    |coef2 E|) per update, an earlier update's allowance carried through the later one."""
    for bname, d, side, sign, ename in SM_RULES:
        if not (sm_hi[d] if side == "hi" else sm_lo[d]):
            continue
        r = CL * dt * dinv[d]                                  # :177-188
        coef1, coef2 = (1.0 - r) / (1.0 + r), 2.0 * r / (1.0 + r) / CL
        st = STAG[bname]
        # the valid box of the component grown by one point (:230-232), in array indices
        a = [ng[x] - 1 for x in range(3)]
        b = [ng[x] + ncell[x] + st[x] + 1 for x in range(3)]
        p = (dom_hi[d] + 1 if side == "hi" else dom_lo[d] - 1) - lo[d]
        if not a[d] <= p < b[d]:
            continue
        idx = [slice(a[x], b[x]) for x in range(3)]
        idx[d] = slice(p, p + 1)
        eidx = list(idx)
        if side == "lo":
            eidx[d] = slice(p + 1, p + 2)
        idx, eidx = tuple(idx), tuple(eidx)
        t1, t2 = coef1 * F[bname][idx], coef2 * F[ename][eidx]
        if tol is not None:
            tol[bname][idx] = abs(coef1) * tol[bname][idx] + 2.0 ** -52 * (np.abs(t1) + np.abs(t2))
        F[bname][idx] = t1 + t2 if sign > 0 else t1 - t2


def _v(name, ncell, ng, shift=(0, 0, 0)):
    """The valid box of component `name`, shifted."""
    st = STAG[name]
    return tuple(slice(ng[d] + shift[d], ng[d] + ncell[d] + st[d] + shift[d]) for d in range(3))


def evolve_b(F, ncell, ng, dt, dinv):
    idx, idy, idz = dinv
    Ex, Ey, Ez = F["Ex"], F["Ey"], F["Ez"]
    v = _v("Bx", ncell, ng)
    F["Bx"][v] = F["Bx"][v] + (dt * (idz * (Ey[_v("Bx", ncell, ng, (0, 0, 1))] - Ey[v])) -
                               dt * (idy * (Ez[_v("Bx", ncell, ng, (0, 1, 0))] - Ez[v])))
    v = _v("By", ncell, ng)
    F["By"][v] = F["By"][v] + (dt * (idx * (Ez[_v("By", ncell, ng, (1, 0, 0))] - Ez[v])) -
                               dt * (idz * (Ex[_v("By", ncell, ng, (0, 0, 1))] - Ex[v])))
    v = _v("Bz", ncell, ng)
    F["Bz"][v] = F["Bz"][v] + (dt * (idy * (Ex[_v("Bz", ncell, ng, (0, 1, 0))] - Ex[v])) -
                               dt * (idx * (Ey[_v("Bz", ncell, ng, (1, 0, 0))] - Ey[v])))


def evolve_e(F, ncell, ng, dt, dinv):
    """No current.  Every valid point, the nodal ones on the faces included: they read the guard plane of B."""
    idx, idy, idz = dinv
    Bx, By, Bz = F["Bx"], F["By"], F["Bz"]
    c2 = CL * CL
    v = _v("Ex", ncell, ng)
    F["Ex"][v] = F["Ex"][v] + c2 * dt * (-(idz * (By[v] - By[_v("Ex", ncell, ng, (0, 0, -1))])) +
                                         (idy * (Bz[v] - Bz[_v("Ex", ncell, ng, (0, -1, 0))])))
    v = _v("Ey", ncell, ng)
    F["Ey"][v] = F["Ey"][v] + c2 * dt * (-(idx * (Bz[v] - Bz[_v("Ey", ncell, ng, (-1, 0, 0))])) +
                                         (idz * (Bx[v] - Bx[_v("Ey", ncell, ng, (0, 0, -1))])))
    v = _v("Ez", ncell, ng)
    F["Ez"][v] = F["Ez"][v] + c2 * dt * (-(idy * (Bx[v] - Bx[_v("Ez", ncell, ng, (0, -1, 0))])) +
                                         (idx * (By[v] - By[_v("Ez", ncell, ng, (-1, 0, 0))])))


def wrap_sources(n, ncell, st, ng):
    """For every array index along a periodic direction: itself if valid, else its periodic image among the valid cells."""
    g = np.arange(n) - ng
    return np.where((g >= 0) & (g < ncell + st), g, np.mod(g, ncell)) + ng


def periodic_fill(F, names, ncell, ng, periodic):
    for name in names:
        for d in range(3):
            if periodic[d]:
                F[name][...] = np.take(F[name], wrap_sources(F[name].shape[d], ncell[d], STAG[name][d], ng[d]), axis=d)


def pec_faces(F, names, ncell, ng, bc_lo, bc_hi):
    """What the valid points see of a PEC wall: the components of `names` that vanish on it (tangential E, normal B) are
    zero on the face."""
    for d in range(3):
        for face, bc in ((ng[d], bc_lo[d]), (ng[d] + ncell[d], bc_hi[d])):
            if bc != PEC:
                continue
            for c, name in enumerate(names):
                if (name[0] == "E") == (c != d):
                    idx = [slice(None)] * 3
                    idx[d] = face
                    F[name][tuple(idx)] = 0.0


def model_run(F0, ncell, ng, dt, dinv, bc_lo, bc_hi, steps):
    F = {k: a.copy() for k, a in F0.items()}
    periodic = [bc_lo[d] == P for d in range(3)]
    sm_lo, sm_hi = [bc_lo[d] == S for d in range(3)], [bc_hi[d] == S for d in range(3)]
    lo, dom_lo, dom_hi = [-g for g in ng], (0, 0, 0), [n - 1 for n in ncell]
    for _ in range(steps):
        evolve_b(F, ncell, ng, 0.5 * dt, dinv)
        pec_faces(F, BN, ncell, ng, bc_lo, bc_hi)
        sm_apply(F, lo, ncell, ng, dt, dinv, dom_lo, dom_hi, sm_lo, sm_hi)   # the full step, after the first half only
        periodic_fill(F, BN, ncell, ng, periodic)
        evolve_e(F, ncell, ng, dt, dinv)
        pec_faces(F, EN, ncell, ng, bc_lo, bc_hi)
        periodic_fill(F, EN, ncell, ng, periodic)
        evolve_b(F, ncell, ng, 0.5 * dt, dinv)
        pec_faces(F, BN, ncell, ng, bc_lo, bc_hi)
    return F


def model_energy(F, ncell, ng, dx):
    """field_energy's formula (warpx_amd/sim.py) on the model's arrays."""
    def sumsq(name):
        x = F[name][tuple(slice(ng[d], ng[d] + ncell[d]) for d in range(3))].astype(np.longdouble)
        return float(np.sum(x * x))
    dV = dx[0] * dx[1] * dx[2]
    return (0.5 * sum(sumsq(n) for n in EN) * plasma.EP0 * dV, 0.5 * sum(sumsq(n) for n in BN) / plasma.MU0 * dV)


# ---- test 1: the kernel against sm_apply ---------------------------------------------------------------------------------

BRICKS = {"small": ((5, 4, 6), False), "long_rows": ((70, 3, 3), True)}   # (70, 3, 3): a row is longer than a wave; padded rows
ALL, NONE = (1, 1, 1), (0, 0, 0)


def _one(d, hi):
    f = [0, 0, 0]
    f[d] = 1
    return (NONE, tuple(f)) if hi else (tuple(f), NONE)


# name -> (sm_lo, sm_hi, where the brick sits: "domain" = it is the domain, "inside" = strictly inside a larger one,
#          "top_of_z" = the upper of two bricks along z)
SELECTIONS = {"all_six": (ALL, ALL, "domain"), "lo_only": (ALL, NONE, "domain"),
              "inside_a_larger_domain": (ALL, ALL, "inside"), "hi_end_of_a_z_split": ((0, 0, 1), (0, 0, 1), "top_of_z")}
for _d in range(3):
    for _hi in (0, 1):
        SELECTIONS["%s_%s" % ("xyz"[_d], "hi" if _hi else "lo")] = _one(_d, _hi) + ("domain",)


@pytest.mark.parametrize("selection", sorted(SELECTIONS))
@pytest.mark.parametrize("brick", sorted(BRICKS))
def test_kernel_against_the_reference_formulas(product, brick, selection):
    ncell, pad = BRICKS[brick]
    sm_lo, sm_hi, where = SELECTIONS[selection]
    ng = (3, 3, 3)
    if where == "domain":
        lo_valid, dom_lo, dom_hi = (0, 0, 0), (0, 0, 0), tuple(n - 1 for n in ncell)
    elif where == "inside":
        lo_valid, dom_lo, dom_hi = (20, 20, 20), (0, 0, 0), tuple(20 + n + 19 for n in ncell)
    else:
        lo_valid, dom_lo, dom_hi = (0, 0, ncell[2]), (0, 0, 0), (ncell[0] - 1, ncell[1] - 1, 2 * ncell[2] - 1)
    dx = np.array([1.0e-6, 1.3e-6, 0.7e-6])
    dinv = 1.0 / dx
    dt = H.yee_dt(dx, 0.95)
    rng = np.random.default_rng(2024)
    dev, F = {}, {}
    for name in EN + BN:
        f = FieldArray(ncell, STAG[name], ng, H.DEVICE, lo_valid, pad=pad)
        F[name] = rng.standard_normal(f.n) * (CL if name[0] == "E" else 1.0)
        dev[name] = f.from_numpy(F[name])
    before = {k: a.copy() for k, a in F.items()}
    tol = {n: np.zeros_like(F[n]) for n in BN}
    lo = [lo_valid[d] - ng[d] for d in range(3)]
    sm_apply(F, lo, ncell, ng, dt, dinv, dom_lo, dom_hi, sm_lo, sm_hi, tol)

    i32 = lambda v: (C.c_int32 * 3)(*[int(x) for x in v])   # noqa: E731
    product.apply_silver_mueller(field_triplet([dev[n] for n in EN]), field_triplet([dev[n] for n in BN]), dt, H.d3(dinv),
                                 i32(dom_lo), i32(dom_hi), i32(sm_lo), i32(sm_hi), None)
    product.device_synchronize()

    touched = 0
    for n in EN:
        assert np.array_equal(dev[n].to_numpy(), before[n]), n                      # E is only read
    for n in BN:
        got = dev[n].to_numpy()
        off = tol[n] == 0.0
        assert np.array_equal(got[off], before[n][off]), n                          # outside the planes: bit for bit
        err = np.abs(got - F[n])
        print(f"{brick} {selection} {n}: {np.count_nonzero(~off)} points updated, "
              f"max |err| / allowance = {np.max(err[~off] / tol[n][~off]) if np.any(~off) else 0.0:.3g}")
        assert np.all(err <= tol[n]), n
        touched += np.count_nonzero(~off)
    # the planes are where they should be: none inside a larger domain, one face of the upper brick, edges counted once
    g = [n + 2 for n in ncell]   # points of the grown box along a cell-centred direction (one more along the nodal one)
    plane = lambda c, d: np.prod([g[x] + (1 if x == c else 0) for x in range(3) if x != d])   # noqa: E731
    want = 0
    if where != "inside":
        for c in range(3):
            d1, d2 = [d for d in range(3) if d != c]
            n1 = sm_lo[d1] + sm_hi[d1] if where == "domain" or d1 != 2 else sm_hi[d1]
            n2 = sm_lo[d2] + sm_hi[d2] if where == "domain" or d2 != 2 else sm_hi[d2]
            edge = g[3 - d1 - d2] + 1   # points of an edge shared by a d1 plane and a d2 plane (it runs along c, nodal)
            want += n1 * plane(c, d1) + n2 * plane(c, d2) - n1 * n2 * edge
    assert touched == want, (touched, want)
    if where == "inside":
        for n in BN:
            assert np.array_equal(dev[n].to_numpy(), before[n]), n


def test_kernel_refuses_what_it_does_not_do(product):
    ncell, ng = (4, 4, 4), (2, 2, 2)
    Y = [FieldArray(ncell, STAG[n], ng, H.DEVICE) for n in EN + BN]
    i32 = lambda v: (C.c_int32 * 3)(*v)   # noqa: E731
    args = (1e-16, H.d3((1e6, 1e6, 1e6)), i32((0, 0, 0)), i32((3, 3, 3)), i32(ALL), i32(ALL), None)
    product.apply_silver_mueller(field_triplet(Y[:3]), field_triplet(Y[3:]), *args)          # the Yee staggering: fine
    nodal = [FieldArray(ncell, (1, 1, 1), ng, H.DEVICE) for _ in range(3)]
    assert product._apply_silver_mueller(field_triplet(Y[:3]), field_triplet(nodal), *args) == -3    # WXA_ERR_UNSUPPORTED
    assert product._apply_silver_mueller(field_triplet(nodal), field_triplet(Y[3:]), *args) == -3
    raw = product._dll["wxa_apply_silver_mueller"]   # a binding of its own whose pointer arguments may be null
    raw.restype, raw.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_double] + [C.c_void_p] * 6
    Ev, Bv = field_triplet(Y[:3]), field_triplet(Y[3:])
    ptr = lambda a: C.cast(a, C.c_void_p)   # noqa: E731
    rest = [ptr(a) for a in args[1:-1]] + [None]
    assert raw(ptr(Ev), ptr(Bv), 1e-16, *rest) == 0
    assert raw(None, ptr(Bv), 1e-16, *rest) == -1                                                     # WXA_ERR_INVALID_ARG
    assert raw(ptr(Ev), None, 1e-16, *rest) == -1
    assert raw(ptr(Ev), ptr(Bv), 1e-16, None, *rest[1:]) == -1
    product.device_synchronize()


# ---- tests 2 and 4: the step against the model, one brick and several ---------------------------------------------------

STEP_NCELL = (16, 12, 20)
STEP_LO, STEP_HI = (0.0, 0.0, 0.0), (16 * 1.0e-6, 12 * 1.3e-6, 20 * 0.7e-6)
STEPS = 120
#        (x, y, z) at the lo faces, at the hi faces
CASES = {"sss": ((S, S, S), (S, S, S)), "pps": ((P, P, S), (P, P, S)), "sps": ((S, P, S), (S, P, S)),
         "psp": ((P, S, P), (P, S, P)), "spp": ((S, P, P), (S, P, P)), "pp_s_pec": ((P, P, S), (P, P, PEC))}


def make_sim(product, bc, **kw):
    return WarpXSim(product, STEP_NCELL, STEP_LO, STEP_HI, cfl=0.95, field_boundary_lo=bc[0], field_boundary_hi=bc[1], **kw)


def wave_packet(shapes, ng, bc_lo):
    """A smooth packet with random phases in all six components, guards included; along a periodic direction the guards
    and the upper nodal point hold their periodic images exactly (the index is wrapped before the formula is applied)."""
    rng = np.random.default_rng(7)
    F = {}
    for name in EN + BN:
        st = STAG[name]
        x = []
        for d in range(3):
            g = np.arange(shapes[name][d]) - ng[d]
            if bc_lo[d] == P:
                g = np.mod(g, STEP_NCELL[d])
            x.append((g + 0.5 * (1 - st[d])) / STEP_NCELL[d])
        X, Y, Z = np.meshgrid(*x, indexing="ij")
        a = np.zeros(X.shape)
        for m in ((1, 1, 2), (2, 1, 1), (1, 2, 3)):
            ph = rng.uniform(0.0, 2.0 * np.pi)
            a += np.sin(2.0 * np.pi * (m[0] * X + m[1] * Y + m[2] * Z) + ph)
        env = np.sin(np.pi * X) ** 2 * np.sin(np.pi * Y) ** 2 * np.sin(np.pi * Z) ** 2
        F[name] = a * env * (CL if name[0] == "E" else 1.0)
    return F


_step_cache = {}


def step_case(product, case):
    """One brick: the product's fields after STEPS steps (with guards), the model's, and what both started from."""
    if case not in _step_cache:
        bc = CASES[case]
        sim = make_sim(product, bc)
        views = {n: sim.field_view(n) for n in EN + BN}
        ng = tuple(views["Ex"].ng)
        assert all(tuple(v.ng) == ng for v in views.values())
        F0 = wave_packet({n: tuple(v.n) for n, v in views.items()}, ng, bc[0])
        for n in EN + BN:
            sim.set_field(n, F0[n])
        dt = sim.dt
        sim.evolve(STEPS)
        got = {n: sim.field_valid(n) for n in EN + BN}
        sim.close()
        dinv = [1.0 / ((STEP_HI[d] - STEP_LO[d]) / STEP_NCELL[d]) for d in range(3)]
        assert abs(dt - H.yee_dt([1.0 / v for v in dinv], 0.95)) < 1e-12 * dt
        M = model_run(F0, STEP_NCELL, ng, dt, dinv, bc[0], bc[1], STEPS)
        want = {n: M[n][_v(n, STEP_NCELL, ng)] for n in EN + BN}
        peak = max(max(np.max(np.abs(F0[n])) for n in EN), CL * max(np.max(np.abs(F0[n])) for n in BN))
        _step_cache[case] = {"got": got, "want": want, "F0": F0, "ng": ng, "peak": peak}
    return _step_cache[case]


@pytest.mark.parametrize("case", sorted(CASES))
def test_step_parity_with_the_model(product, case):
    r = step_case(product, case)
    for n in EN + BN:
        scale = r["peak"] / (1.0 if n[0] == "E" else CL)
        err = float(np.max(np.abs(r["got"][n] - r["want"][n])) / scale)
        left = float(np.max(np.abs(r["want"][n])) / scale)
        print(f"{case} {n}: max |product - model| / peak = {err:.3g} (|field| / peak after {STEPS} steps: {left:.3g})")
        assert err < 1e-12, (case, n)


def run_bricks(product, nb, bc, F0, steps):
    """The step_case run cut into nb bricks (threads of this process over ThreadBrickTransport)."""
    nranks = nb[0] * nb[1] * nb[2]
    bn = [STEP_NCELL[d] // nb[d] for d in range(3)]
    shared = thread_transport_state()
    results, errors = [None] * nranks, []

    def brick(rank):
        shared["turn"].acquire()
        try:
            coord = brick_coord(rank, nb)
            tr = ThreadBrickTransport(rank, nranks, shared)
            sim = make_sim(product, bc, nbricks=nb, coord=coord, comm=tr.comm)
            for n in EN + BN:
                shape = tuple(sim.field_view(n).n)
                sim.set_field(n, np.ascontiguousarray(
                    F0[n][tuple(slice(coord[d] * bn[d], coord[d] * bn[d] + shape[d]) for d in range(3))]))
            sim.evolve(steps)
            results[rank] = {"coord": coord, "fields": {n: sim.field_valid(n) for n in EN + BN}, "exchanges": tr.n_exchanges}
            sim.close()
        except Exception as e:  # noqa: BLE001
            errors.append((rank, repr(e)))
            thread_transport_abort(shared)
        finally:
            shared["turn"].release()

    threads = [threading.Thread(target=brick, args=(r,)) for r in range(nranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    assert not errors, errors
    assert all(r is not None for r in results)
    return results, bn


@pytest.mark.parametrize("case,nb", [("pps", (1, 1, 2)), ("sps", (2, 1, 2))])
def test_bricks_apply_the_boundary_at_the_domain_faces_only(product, case, nb):
    one = step_case(product, case)
    results, bn = run_bricks(product, nb, CASES[case], one["F0"], STEPS)
    assert all(r["exchanges"] > 0 for r in results)
    for n in EN + BN:
        scale = one["peak"] / (1.0 if n[0] == "E" else CL)
        for r in results:
            c, a = r["coord"], r["fields"][n]
            full = one["got"][n][tuple(slice(c[d] * bn[d], c[d] * bn[d] + a.shape[d]) for d in range(3))]
            if H.ON_GPU:
                assert float(np.max(np.abs(a - full)) / scale) < 1e-12, (n, c)
            else:
                assert np.array_equal(a, full), (n, c)


# ---- test 3: it absorbs ---------------------------------------------------------------------------------------------------

def test_a_pulse_leaves_the_box(product):
    """A z-independent column of Ez spreads in x and y and leaves through Silver-Mueller faces all around: after 150 steps
    less than 1e-3 of its energy is left (the model: 9.6e-7 with these faces, 0.991 in a periodic box and between mirrors)."""
    ncell, h = (24, 20, 8), 1.0e-6
    bc = ((S, S, S), (S, S, S))
    hi = tuple(n * h for n in ncell)
    sim = WarpXSim(product, ncell, (0.0, 0.0, 0.0), hi, cfl=0.95, field_boundary_lo=bc[0], field_boundary_hi=bc[1])
    views = {n: sim.field_view(n) for n in EN + BN}
    ng = tuple(views["Ex"].ng)
    F0 = {n: np.zeros(tuple(v.n)) for n, v in views.items()}
    shape = F0["Ez"].shape     # Ez is nodal in x and y: the point with index i sits at x = i cells
    x = np.arange(shape[0]) - ng[0]
    y = np.arange(shape[1]) - ng[1]
    col = np.exp(-((x[:, None] - ncell[0] / 2) / (ncell[0] / 8)) ** 2 - ((y[None, :] - ncell[1] / 2) / (ncell[1] / 8)) ** 2)
    F0["Ez"][...] = col[:, :, None]
    for n in EN + BN:
        sim.set_field(n, F0[n])
    e0 = sum(field_energy(sim))
    sim.evolve(150)
    e1 = sum(field_energy(sim))
    dt = sim.dt
    sim.close()
    M = model_run(F0, ncell, ng, dt, [1.0 / h] * 3, bc[0], bc[1], 150)
    m0, m1 = sum(model_energy(F0, ncell, ng, [h] * 3)), sum(model_energy(M, ncell, ng, [h] * 3))
    print(f"energy left after 150 steps: product {e1 / e0:.6e}, model {m1 / m0:.6e}")
    assert e1 / e0 < 1e-3
    assert abs(e1 / e0 - m1 / m0) < 1e-9 * (m1 / m0)


# ---- test 5: the deck -------------------------------------------------------------------------------------------------

def _deck_fields(sim, steps):
    sim.evolve(steps)
    out = {n: sim.field_valid(n) for n in EN + BN}
    sim.close()
    return out


def test_deck(product):
    """tests/decks/silver_mueller_3d.inputs through the inputs reader and through the constructor leave the same fields; the
    pulse has left through the far face, where a mirror (pec) sends it back into the box."""
    by_deck = WarpXSim.from_inputs(product, DECK)
    steps = by_deck.max_step
    assert steps == 360
    a = _deck_fields(by_deck, steps)

    sim = WarpXSim(product, (16, 16, 192), (-16e-6, -16e-6, -4.8e-6), (16e-6, 16e-6, 4.8e-6), nox=1, galerkin=1,
                   use_filter=0, cfl=0.95, sort_interval=4, field_boundary_lo=(P, P, S), field_boundary_hi=(P, P, S))
    la = _capi.LaserAntenna()
    for d in range(3):
        la.position[d], la.direction[d], la.polarization[d] = (0.0, 0.0, -3e-6)[d], (0.0, 0.0, 1.0)[d], (0.0, 1.0, 0.0)[d]
    la.e_max, la.wavelength = 1e12, 0.8e-6
    la.waist, la.duration, la.t_peak, la.focal_distance = 6e-6, 5e-15, 15e-15, 3e-6
    product.sim_add_laser(sim._h, C.byref(la))
    b = _deck_fields(sim, steps)
    peak = max(max(np.max(np.abs(a[n])) for n in EN), CL * max(np.max(np.abs(a[n])) for n in BN))
    for n in EN + BN:
        if H.ON_GPU:
            assert float(np.max(np.abs(a[n] - b[n]))) * (1.0 if n[0] == "E" else CL) <= 1e-12 * peak, n
        else:
            assert np.array_equal(a[n], b[n]), n

    mirror = _deck_fields(WarpXSim.from_inputs(product, DECK, overrides=["boundary.field_hi = periodic periodic pec"]), steps)
    open_peak, mirror_peak = float(np.max(np.abs(a["Ey"]))), float(np.max(np.abs(mirror["Ey"])))
    print(f"peak |Ey| left in the box after {steps} steps: Silver-Mueller {open_peak:.6e} V/m, mirror {mirror_peak:.6e} V/m, "
          f"ratio {open_peak / mirror_peak:.4g}")
    assert mirror_peak > 0.1e12            # the mirror run does hold the pulse (e_max = 1e12)
    assert open_peak < 0.1 * mirror_peak
