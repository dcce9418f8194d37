"""The particle-grid operations written from their definitions, in numpy at extended precision (np.longdouble).

What the oracle (oracle/pic_kernels.hpp) and the HIP kernels (csrc/shapes.hpp) state as piecewise polynomials per
order is stated here once, as the cardinal B-spline by the Cox-de Boor recursion, and every operation is a dense sum
over ALL points of the arrays it is handed: no stencil origin, no shift, no table of coefficients.  A wrong quartic
coefficient or a half-cell slip made alike in the two libraries passes every parity test between them; it does not pass
a comparison with this file.

    charge      rho(i,j,k)   += q w / dV . S_n(X - i) S_n(Y - j) S_n(Z - k)                      (rho nodal)
    gather      F_p           = sum_ijk F(i,j,k) . prod_d S_{n_d}(X_d - P_d(i_d))
                                P_d(i) = i on a nodal direction of the component, i + 1/2 on a cell-centred one;
                                n_d = n, or n - 1 along the cell-centred directions with Galerkin interpolation
                                (order 0: the top-hat on [-1/2, 1/2))
    direct J    J_c(i,j,k)   += q w v_c / dV . prod_d S_n(X_d - P_d(i_d))   at x + relative_time . v
    Esirkepov   W_c           = DS_c (S0_a S0_b + DS_a S0_b / 2 + S0_a DS_b / 2 + DS_a DS_b / 3)    (Esirkepov 2001, eq. 31)
                J_c(i + 1/2) - J_c(i - 1/2) = -(dx_c / dt) q w W_c(i) / dV, summed from the low side

X is the position in index units of the geometry the kernels are handed: (x - g.xyzmin) . g.dinv + g.lo, the one double
precision map the model shares with the libraries (formed from prob_lo and a global index instead, the rounding of
xyzmin returns: 1e-12 at a 2 mm offset; and the top-hat of the order-1 Galerkin gather is discontinuous, so a particle ON
a node belongs to the cell this very product says).  Everything behind it is np.longdouble.

Vectorised over a few hundred particles as one dense weight matrix per direction, contracted with einsum.
"""
import numpy as np

from warpx_amd import plasma
from warpx_amd.containers import STAG

LD = np.longdouble


def bspline(n, t):
    """The cardinal B-spline of degree n (0..4) centred on 0, support [-(n+1)/2, (n+1)/2), by the Cox-de Boor recursion on
    the uniform knots k_i = i - (n+1)/2:  N_{i,0} = [k_i <= t < k_{i+1}],
    N_{i,p}(t) = ((t - k_i) N_{i,p-1}(t) + (k_{i+p+1} - t) N_{i+1,p-1}(t)) / p,  B_n = N_{0,n}."""
    t = np.asarray(t, dtype=LD)
    half = LD(n + 1) / 2
    knot = [LD(i) - half for i in range(n + 2)]
    level = [((t >= knot[i]) & (t < knot[i + 1])).astype(LD) for i in range(n + 1)]
    for p in range(1, n + 1):
        level = [((t - knot[i]) * level[i] + (knot[i + p + 1] - t) * level[i + 1]) / LD(p) for i in range(n + 1 - p)]
    return level[0]


def index_coordinate(x, g, d):
    """Position in index units along d: the geometry's own map (see the module's docstring)."""
    x = np.asarray(x, dtype=np.float64)
    return ((x - np.float64(g.xyzmin[d])) * np.float64(g.dinv[d])).astype(LD) + LD(int(g.lo[d]))


def _coordinate_ld(x, g, d):
    """The same map for a position that only exists at extended precision (x + relative_time v)."""
    return (np.asarray(x, dtype=LD) - LD(g.xyzmin[d])) * LD(g.dinv[d]) + LD(int(g.lo[d]))


def weights(n, X, lo, npts, nodal):
    """W[p, i] = S_n(X_p - P(lo + i)) for the npts points of an array that starts at index lo."""
    P = np.arange(lo, lo + npts).astype(LD) + (LD(0) if nodal else LD(1) / 2)
    return bspline(n, X[:, None] - P[None, :])


def velocities(parts):
    u = [np.asarray(parts[4 + d], dtype=LD) for d in range(3)]
    gamma = np.sqrt(1 + (u[0] ** 2 + u[1] ** 2 + u[2] ** 2) / LD(plasma.C_LIGHT) ** 2)
    return [ud / gamma for ud in u]


def _inv_volume(g):
    return LD(g.dinv[0]) * LD(g.dinv[1]) * LD(g.dinv[2])


def _inside(W):
    """Every particle's weights along a direction sum to one: its stencil lies inside the array."""
    assert np.max(np.abs(W.sum(axis=1) - 1)) < 1e-17, "a stencil leaves the array: more guard cells"


def charge(parts, g, field, q, order, x=None):
    """rho on the points of `field` (a FieldArray: index origin, shape and staggering), as [i, j, k] with guards."""
    pos = parts[:3] if x is None else x
    W = []
    for d in range(3):
        X = index_coordinate(pos[d], g, d) if x is None else _coordinate_ld(pos[d], g, d)
        W.append(weights(order, X, field.lo[d], field.n[d], field.stag[d] == 1))
        _inside(W[d])
    amp = LD(q) * np.asarray(parts[3], dtype=LD) * _inv_volume(g)
    return np.einsum("p,pi,pj,pk->ijk", amp, *W)


def gather(parts, g, field, name, order, galerkin):
    """The component `name` ("Ex" .. "Bz") at the particles."""
    W = []
    for d in range(3):
        nodal = STAG[name][d] == 1
        n = order - 1 if (galerkin and not nodal) else order
        W.append(weights(n, index_coordinate(parts[d], g, d), field.lo[d], field.n[d], nodal))
        _inside(W[d])
    F = field.to_numpy().astype(LD)
    return np.einsum("pi,pij->p", W[0], np.einsum("pj,pk,ijk->pij", W[1], W[2], F))


def deposit_direct(parts, g, J, q, relative_time, order):
    """[jx, jy, jz] on the points of the three FieldArrays J."""
    v = velocities(parts)
    X = [_coordinate_ld(np.asarray(parts[d], dtype=LD) + LD(relative_time) * v[d], g, d) for d in range(3)]
    out = []
    for c, f in enumerate(J):
        W = [weights(order, X[d], f.lo[d], f.n[d], f.stag[d] == 1) for d in range(3)]
        for Wd in W:
            _inside(Wd)
        amp = LD(q) * np.asarray(parts[3], dtype=LD) * v[c] * _inv_volume(g)
        out.append(np.einsum("p,pi,pj,pk->ijk", amp, *W))
    return out


def esirkepov_positions(parts, dt, relative_time):
    """(x_old, x_new) of the step the current belongs to: x_new = x + (relative_time + dt/2) v, x_old = x_new - dt v (with
    relative_time = -dt/2 the stored position is the new one)."""
    v = velocities(parts)
    new = [np.asarray(parts[d], dtype=LD) + (LD(relative_time) + LD(dt) / 2) * v[d] for d in range(3)]
    old = [new[d] - LD(dt) * v[d] for d in range(3)]
    return old, new


def deposit_esirkepov(parts, g, J, q, dt, relative_time, order):
    """[jx, jy, jz] on the points of the three FieldArrays J (Yee staggering: J_c cell-centred along c, nodal across)."""
    old, new = esirkepov_positions(parts, dt, relative_time)
    out = []
    for c, f in enumerate(J):
        assert tuple(f.stag) == tuple(1 if d != c else 0 for d in range(3))
        # nodal weights on the index range of this component's array: node i and the point i + 1/2 of J_c share an index
        S0, DS = [], []
        for d in range(3):
            w_old = weights(order, _coordinate_ld(old[d], g, d), f.lo[d], f.n[d], True)
            w_new = weights(order, _coordinate_ld(new[d], g, d), f.lo[d], f.n[d], True)
            _inside(w_old)
            _inside(w_new)
            S0.append(w_old)
            DS.append(w_new - w_old)
        a, b = [d for d in range(3) if d != c]
        third, half = LD(1) / 3, LD(1) / 2
        cross = (np.einsum("pa,pb->pab", S0[a], S0[b]) + half * np.einsum("pa,pb->pab", DS[a], S0[b])
                 + half * np.einsum("pa,pb->pab", S0[a], DS[b]) + third * np.einsum("pa,pb->pab", DS[a], DS[b]))
        amp = -(1 / LD(g.dinv[c])) / LD(dt) * LD(q) * np.asarray(parts[3], dtype=LD) * _inv_volume(g)
        Wc = np.einsum("pc,pab->cab", amp[:, None] * DS[c], cross)      # -(dx_c / dt) q w W_c / dV, summed over particles
        Jc = np.cumsum(Wc, axis=0)                                       # J_c(i + 1/2) = sum over nodes <= i
        out.append(np.moveaxis(Jc, 0, c))                                # axes (c, a, b) -> (x, y, z)
    return out


def boris_rotation(u0, B, q, m, dt):
    """The Boris push with E = 0 (Boris 1970; Birdsall & Langdon 4-4): u' = u + (u + u x t) x s, t = q dt / (2 m gamma) B,
    s = 2 t / (1 + t^2)."""
    u0 = [np.asarray(v, dtype=LD) for v in u0]
    gamma = np.sqrt(1 + (u0[0] ** 2 + u0[1] ** 2 + u0[2] ** 2) / LD(plasma.C_LIGHT) ** 2)
    k = LD(q) * LD(dt) / (2 * LD(m)) / gamma
    t = [k * np.asarray(b, dtype=LD) for b in B]
    s = [2 * td / (1 + t[0] ** 2 + t[1] ** 2 + t[2] ** 2) for td in t]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    up = [u0[d] + cd for d, cd in enumerate(cross(u0, t))]
    return [u0[d] + cd for d, cd in enumerate(cross(up, s))]


def max_rel_err(a, b):
    """max |a - b| / max |b|, b the model's (extended-precision) value."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), LD(1e-300)))


# ---- a library against the model ---------------------------------------------------------------------------------------
# One function for the oracle (host arrays) and for the HIP library (device arrays; tiles=True: the LDS-tile kernels behind
# a cell sort), so that tests/test_spline_model_cpu.py and tests/test_geometry_gpu.py measure the same thing.

OPS = ("charge", "gather_E_galerkin", "gather_E_plain", "gather_B_galerkin", "gather_B_plain", "direct", "esirkepov",
       "esirkepov_slow")
U_SCALE = {"direct": 1.0, "esirkepov": 1.0, "esirkepov_slow": 0.003}


def case_particles(case, op, n, seed, lattice):
    """n particles in the box of `case` (a tests.helpers.GeomCase): uniform, or on the half-cell lattice (nodes, cell
    centres and faces in every combination); momenta as the operation needs them."""
    parts = case.random_particles(n, seed, U_SCALE.get(op, 0.01))
    if lattice:
        rng = np.random.default_rng(seed + 1)
        for d in range(3):
            parts[d] = case.plo[d] + rng.integers(0, 2 * case.ncell[d], n) * (0.5 * case.dx[d])
    if op.startswith("gather_E"):
        for r in (4, 5, 6):
            parts[r] = np.zeros(n)
    return parts


def library_error(lib, device, op, order, case, parts, tiles=False):
    """The operation `op` of `lib` on `parts` in the box `case`, against the model: max-norm relative error."""
    import ctypes as C

    from tests import helpers as H
    from warpx_amd import _capi
    from warpx_amd.containers import ParticleArrays, field_triplet
    on_device = device != "cpu"
    q, m = -plasma.Q_E, plasma.M_E
    dt = H.yee_dt(case.dx)
    pa = ParticleArrays.from_numpy(parts, device)
    ws = None
    if tiles:
        ws = C.c_void_p()
        lib.workspace_create(C.byref(ws))
        srt = ParticleArrays(pa.np, device)
        lib.sort_particles_by_cell(C.byref(pa.view), C.byref(srt.view), *case.sort_args(), ws, None)
        lib.device_synchronize()
        pa, parts = srt, list(srt.to_numpy())
    try:
        if op == "charge":
            ng = order + 2
            rho = case.field("rho", ng, device, pad=on_device)
            g = case.geom(ng)
            lib.deposit_charge(C.byref(pa.view), C.byref(rho.view), C.byref(g), plasma.Q_E, order, None)
            if on_device:
                lib.device_synchronize()
            return max_rel_err(rho.to_numpy(), charge(parts, g, rho, plasma.Q_E, order))
        if op.startswith("gather"):
            ng = H.guard_depths(order)[0]
            galerkin = 1 if op.endswith("galerkin") else 0
            of_e = op.startswith("gather_E")
            E = case.random_fields(("Ex", "Ey", "Ez"), ng, 10, scale=1e11 if of_e else 0.0)
            B = case.random_fields(("Bx", "By", "Bz"), ng, 11, scale=0.0 if of_e else 1e4)
            Ed, Bd = (H.clone_fields(f, device, True) for f in (E, B)) if on_device else (E, B)
            g = case.geom(ng)
            if tiles:
                lib.gather_push_ws(C.byref(pa.view), field_triplet(Ed), field_triplet(Bd), C.byref(g), q, m, dt, order,
                                   galerkin, _capi.PUSHER_BORIS, 0, ws, None)
            else:
                lib.push_p(C.byref(pa.view), field_triplet(Ed), field_triplet(Bd), C.byref(g), q, m, dt, order, galerkin,
                           _capi.PUSHER_BORIS, None)
            if on_device:
                lib.device_synchronize()
            got = pa.to_numpy()[4:7]
            if of_e:   # u = 0 and B = 0: the Boris push leaves q dt / m . E
                want = [LD(q) * LD(dt) / LD(m) * gather(parts, g, f, name, order, galerkin)
                        for f, name in zip(E, ("Ex", "Ey", "Ez"))]
                return max(max_rel_err(got[c], want[c]) for c in range(3))
            u0 = [np.asarray(parts[4 + c], dtype=LD) for c in range(3)]
            want = boris_rotation(u0, [gather(parts, g, f, name, order, galerkin) for f, name in zip(B, ("Bx", "By", "Bz"))],
                                  q, m, dt)
            turn = max(np.max(np.abs(want[c] - u0[c])) for c in range(3))
            return float(max(np.max(np.abs(got[c].astype(LD) - want[c])) for c in range(3)) / turn)
        algo = _capi.DEPOSIT_DIRECT if op == "direct" else _capi.DEPOSIT_ESIRKEPOV
        _, ng_depos, ng_j = H.guard_depths(order, use_filter=True)
        J = [case.field(n, ng_j, device, pad=on_device) for n in ("jx", "jy", "jz")]
        g = case.geom(ng_depos)
        lib.deposit_current(C.byref(pa.view), field_triplet(J), C.byref(g), q, dt, -0.5 * dt, order, algo, ws, None)
        if on_device:
            lib.device_synchronize()
        want = (deposit_direct(parts, g, J, q, -0.5 * dt, order) if op == "direct"
                else deposit_esirkepov(parts, g, J, q, dt, -0.5 * dt, order))
        return max(max_rel_err(f.to_numpy(), w) for f, w in zip(J, want))
    finally:
        if ws is not None:
            lib.workspace_destroy(ws)


# The suite's parity gates (HIP against oracle): the model's gates are never looser.
PARITY_GATE = {op: 1e-12 for op in OPS}
PARITY_GATE["esirkepov_slow"] = 2e-11

# Oracle against model on the CPU: the worst of the cases of tests/test_spline_model_cpu.py per operation and order
# (profiles/round10/README.md).  Each gate is ten times its figure.
MEASURED = {
    "charge": {1: 2.2e-16, 2: 2.7e-16, 3: 4.8e-16, 4: 6.4e-16},
    "gather_E_galerkin": {1: 3.1e-16, 2: 4.6e-16, 3: 7.2e-16, 4: 8.8e-16},
    "gather_E_plain": {1: 3.5e-16, 2: 5.1e-16, 3: 6.2e-16, 4: 1.2e-15},
    "gather_B_galerkin": {1: 2.1e-16, 2: 3.4e-16, 3: 4.9e-16, 4: 4.8e-16},
    "gather_B_plain": {1: 5.7e-16, 2: 3.9e-16, 3: 5.4e-16, 4: 7.9e-16},
    "direct": {1: 6.2e-15, 2: 4.9e-15, 3: 4.8e-15, 4: 5.3e-15},
    "esirkepov": {1: 7.1e-15, 2: 5.2e-15, 3: 6.5e-15, 4: 4.6e-15},
    "esirkepov_slow": {1: 1.1e-12, 2: 5.1e-13, 3: 6.2e-13, 4: 7.6e-13},
}


def gate(op, order):
    return min(10.0 * MEASURED[op][order], PARITY_GATE[op])
