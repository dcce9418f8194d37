"""The HIP particle kernels in boxes that are not the suite's usual one, and against the definitions.

tests/test_kernels_gpu.py runs every particle kernel in H.geom_for's geometry: prob_lo = -LX/2, box index origin 0,
cell_lo = 0, box sizes that are multiples of 4.  The tile kernels do their arithmetic in exactly these quantities
(tg.cell_lo + ti * 8 + LO, the sort key's (x - plo) * dinv, partial last tiles, the face test of the periodic wrap), and
a brick of a multi-brick run or a moving window hands them other values.  Here: one table of boxes with odd sizes,
negative and large index origins, a 2 mm physical offset and a single-cell direction; every kernel on each of them
against the CPU oracle at the suite's gates, particles on the lattice of nodes, cell centres and faces, and the kernels
against tests/spline_model.py without the oracle in between."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from tests import spline_model as M
from warpx_amd import _capi, plasma
from warpx_amd.containers import ParticleArrays, field_triplet

pytestmark = pytest.mark.gpu

DEV = H.DEVICE
ESIRKEPOV, DIRECT = _capi.DEPOSIT_ESIRKEPOV, _capi.DEPOSIT_DIRECT

# name: (ncell, box_lo, prob_lo, dx)
BOXES = {
    "13x7x9_at_0": ((13, 7, 9), (0, 0, 0), (-3.25e-6, -1.4e-6, -1.125e-6), (0.5e-6, 0.4e-6, 0.25e-6)),
    "13x7x9_offset": ((13, 7, 9), (5, -3, 100), (1e-6, -3e-6, 2e-3), (0.5e-6, 0.4e-6, 0.25e-6)),
    "17x8x5_negative": ((17, 8, 5), (-3, -16, -7), (2e-6, 5e-6, -1e-6), (0.3e-6, 0.7e-6, 0.45e-6)),
    "9x9x33_far": ((9, 9, 33), (0, 0, 4000), (-2.25e-6, -2.25e-6, -1e-4), (0.5e-6, 0.5e-6, 0.03e-6)),
    "3x2x1": ((3, 2, 1), (0, 0, 0), (-1e-6, 0.0, 3e-6), (0.4e-6, 0.5e-6, 0.6e-6)),
    # 3 x 3 x 4 tiles, two of them interior, partial last tiles in x and z
    "17x24x25": ((17, 24, 25), (3, -5, 64), (-4e-6, 1e-6, -7e-6), (0.5e-6, 0.4e-6, 0.25e-6)),
}
# the same boxes with cells that are powers of two and prob_lo a multiple of them: node positions are exact
POW2_DX = (2.0 ** -21, 2.0 ** -22, 2.0 ** -20)
POW2_PROB_LO = (3 * POW2_DX[0], -7 * POW2_DX[1], 2048 * POW2_DX[2])


def _case(box, pow2=False):
    ncell, box_lo, prob_lo, dx = BOXES[box]
    return H.geom_case(ncell, box_lo, POW2_PROB_LO, POW2_DX) if pow2 else H.geom_case(ncell, box_lo, prob_lo, dx)


def _npart(case):
    return min(6000, 40 * case.ncell[0] * case.ncell[1] * case.ncell[2])


def _sort(product, case, parts, room=0):
    """A workspace with the cell sort of `parts`, and the sorted tile (with `room` free slots behind it)."""
    src = ParticleArrays.from_numpy(parts, DEV)
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    srt = ParticleArrays(src.np + room, DEV)
    view = _capi.ParticleView.from_buffer_copy(srt.view)
    view.np = src.np
    product.sort_particles_by_cell(C.byref(src.view), C.byref(view), *case.sort_args(), ws, None)
    product.device_synchronize()
    return ws, srt


def _displace(case, srt, seed, cells=0.9):
    """Moved by up to `cells` cells since the sort, kept inside the box (as the step loop guarantees)."""
    import torch
    rng = np.random.default_rng(seed)
    for d in range(3):
        srt.data[d] += torch.from_numpy(case.dx[d] * cells * (2 * rng.random(srt.np) - 1)).to(DEV)
        srt.data[d].clamp_(float(case.plo[d]), float(case.below_phi(d)))


def _stragglers(product, ws, tile_kernel):
    n = C.c_int64(-1)
    product.workspace_last_stragglers(ws, tile_kernel, C.byref(n))
    return n.value


def _deposit_against_oracle(oracle, product, case, srt, ws, order, algo, tol):
    """J of the tile kernels (through ws) and of the global kernel, both against the oracle, per component.  Returns how
    many particles the tile kernel left to its global-atomics pass."""
    _, ng_depos, ng_j = H.guard_depths(order, use_filter=True)
    ph = ParticleArrays.from_numpy(list(srt.to_numpy()), "cpu")
    J = [case.field(n, ng_j) for n in ("jx", "jy", "jz")]
    Jt, Jg = H.clone_fields(J, DEV, True), H.clone_fields(J, DEV, True)
    g = case.geom(ng_depos)
    dt = H.yee_dt(case.dx)
    q = -plasma.Q_E
    oracle.deposit_current(C.byref(ph.view), field_triplet(J), C.byref(g), q, dt, -0.5 * dt, order, algo, None, None)
    product.deposit_current(C.byref(srt.view), field_triplet(Jt), C.byref(g), q, dt, -0.5 * dt, order, algo, ws, None)
    stragglers = _stragglers(product, ws, _capi.TILE_DEPOSIT)
    product.deposit_current(C.byref(srt.view), field_triplet(Jg), C.byref(g), q, dt, -0.5 * dt, order, algo, None, None)
    product.device_synchronize()
    for name, a, b, c in zip("xyz", Jt, Jg, J):
        want = c.to_numpy()
        assert np.max(np.abs(want)) > 0
        et, eg = H.max_rel_err(a.to_numpy(), want), H.max_rel_err(b.to_numpy(), want)
        print(f"J{name} tiles {et:.2e} global {eg:.2e}")
        assert et < tol and eg < tol, (name, et, eg)
    return stragglers


def _gather_against_oracle(oracle, product, case, srt, ws, order, galerkin, pusher=_capi.PUSHER_BORIS):
    """PushP (move 0) then PushPX (move 1) on the tile kernels and on the global kernel, against the oracle.  Returns how
    many particles the tile kernel's first launch left to its global-load pass."""
    stragglers = None
    ng, _, _ = H.guard_depths(order)
    E = case.random_fields(("Ex", "Ey", "Ez"), ng, 10, scale=1e11)
    B = case.random_fields(("Bx", "By", "Bz"), ng, 11, scale=1e3)
    Ed, Bd = H.clone_fields(E, DEV, True), H.clone_fields(B, DEV, True)
    ph = ParticleArrays.from_numpy(list(srt.to_numpy()), "cpu")
    pg = ParticleArrays.from_numpy(list(srt.to_numpy()), DEV)
    g = case.geom(ng)
    dt = H.yee_dt(case.dx)
    q, m = -plasma.Q_E, plasma.M_E
    for move, fn in ((0, "push_p"), (1, "gather_push")):
        getattr(oracle, fn)(C.byref(ph.view), field_triplet(E), field_triplet(B), C.byref(g), q, m, dt, order, galerkin,
                            pusher, None)
        product.gather_push_ws(C.byref(srt.view), field_triplet(Ed), field_triplet(Bd), C.byref(g), q, m, dt, order,
                               galerkin, pusher, move, ws, None)
        if stragglers is None:
            stragglers = _stragglers(product, ws, _capi.TILE_GATHER)
        getattr(product, fn)(C.byref(pg.view), field_triplet(Ed), field_triplet(Bd), C.byref(g), q, m, dt, order,
                             galerkin, pusher, None)
        product.device_synchronize()
        want = ph.to_numpy()
        for lib_name, got in (("tiles", srt.to_numpy()), ("global", pg.to_numpy())):
            for row in range(7):
                assert H.max_rel_err(got[row], want[row]) < 1e-12, (lib_name, fn, row)
    return stragglers


# ---- 1. tile and global kernels against the oracle on every box ----------------------------------------------------------

@pytest.mark.parametrize("box", list(BOXES))
@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("algo", [ESIRKEPOV, DIRECT])
@pytest.mark.parametrize("stale,u_scale", [(False, 1.0), (True, 1.0), (False, 0.003)])
def test_deposition_on_every_box(oracle, product, box, order, algo, stale, u_scale):
    """The LDS-tile deposition and the global-atomics kernel against the oracle: fresh sort, a sort that is stale by up to
    0.9 cell, and slow particles (the tile kernel's pair path) at the suite's gates.
    A tile staged in the wrong place costs no accuracy: every particle's frame then leaves it and the global-atomics pass
    deposits the same sums.  So the slow case also counts what the tile kernel handed on: behind a fresh sort only a
    particle that crosses a tile face in this step can leave its frame, under 0.01 cell at 0.003 c -- fewer than one in
    a hundred even if every cell were a face cell."""
    case = _case(box)
    ws, srt = _sort(product, case, case.random_particles(_npart(case), 200 + order, u_scale))
    if stale:
        _displace(case, srt, 5)
    stragglers = _deposit_against_oracle(oracle, product, case, srt, ws, order, algo,
                                         2e-11 if (u_scale != 1.0 and algo == ESIRKEPOV) else 1e-12)
    if u_scale != 1.0:
        assert 0 <= stragglers <= srt.np // 100, stragglers
    product.workspace_destroy(ws)


@pytest.mark.parametrize("box", list(BOXES))
@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("galerkin", [1, 0])
@pytest.mark.parametrize("stale", [False, True])
def test_gather_on_every_box(oracle, product, box, order, galerkin, stale):
    """The LDS-tile gather (move 0 and 1) and the global kernel against the oracle, fresh and stale sort.  Behind a fresh
    sort every stencil lies in its tile's staged points: no particle goes to the global-load pass (a tile staged in the
    wrong place would send all of them there, and that pass gathers the same values)."""
    case = _case(box)
    ws, srt = _sort(product, case, case.random_particles(_npart(case), 300 + order))
    if stale:
        _displace(case, srt, 6)
    stragglers = _gather_against_oracle(oracle, product, case, srt, ws, order, galerkin)
    if not stale:
        assert stragglers == 0
    product.workspace_destroy(ws)


@pytest.mark.parametrize("box", list(BOXES))
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_charge_on_every_box(oracle, product, box, order):
    case = _case(box)
    ng = order + 2
    parts = case.random_particles(_npart(case), 40)
    rho = case.field("rho", ng)
    rhod = rho.copy_to(DEV, True)
    ph, pd = ParticleArrays.from_numpy(parts, "cpu"), ParticleArrays.from_numpy(parts, DEV)
    g = case.geom(ng)
    oracle.deposit_charge(C.byref(ph.view), C.byref(rho.view), C.byref(g), plasma.Q_E, order, None)
    product.deposit_charge(C.byref(pd.view), C.byref(rhod.view), C.byref(g), plasma.Q_E, order, None)
    product.device_synchronize()
    assert H.max_rel_err(rhod.to_numpy(), rho.to_numpy()) < 1e-12


def test_straggler_count_of_a_workspace_without_a_launch(product):
    """wxa_workspace_last_stragglers before any tile launch: 0 for both kernels; another kernel id is an error."""
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    assert _stragglers(product, ws, _capi.TILE_GATHER) == 0 and _stragglers(product, ws, _capi.TILE_DEPOSIT) == 0
    with pytest.raises(_capi.WxaError):
        product.workspace_last_stragglers(ws, 2, C.byref(C.c_int64()))
    product.workspace_destroy(ws)


# ---- 2. particles on the lattice ---------------------------------------------------------------------------------------

def _lattice_particles(case, seed):
    """Every direction draws from: the half-cell lattice (nodes, cell centres), the tile faces (index multiples of 8 from
    box_lo), the box's lower face, and the last double below its upper face.  The first particles are the lower corner, the
    upper corner and the corners of every tile."""
    rng = np.random.default_rng(seed)
    n = _npart(case)
    pos = []
    for d in range(3):
        nc = case.ncell[d]
        half = case.plo[d] + np.arange(2 * nc) * (0.5 * case.dx[d])
        faces = case.plo[d] + np.arange(0, nc, 8) * case.dx[d]
        pool = np.concatenate([half, faces, faces, [case.plo[d], case.below_phi(d)]])
        pos.append(pool[rng.integers(0, pool.size, n)])
    corners = np.array(np.meshgrid(*[np.concatenate([case.plo[d] + np.arange(0, case.ncell[d], 8) * case.dx[d],
                                                     [case.below_phi(d)]]) for d in range(3)], indexing="ij")).reshape(3, -1)
    k = min(corners.shape[1], n)
    for d in range(3):
        pos[d][:k] = corners[d][:k]
    w = 1e9 * (0.5 + rng.random(n))
    return pos + [w] + [0.3 * plasma.C_LIGHT * rng.standard_normal(n) for _ in range(3)]


@pytest.mark.parametrize("box", list(BOXES))
@pytest.mark.parametrize("pow2", [False, True])
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_particles_on_the_lattice(oracle, product, box, pow2, order):
    """Particles on nodes, cell centres, tile faces, the lower corner and one ulp below the upper faces.  The sort returns a
    permutation whose tile-major keys (cell_of restated with plo, dinv and the cell count) do not decrease, every cell
    index inside the box without the clamp having acted; deposition and gather on that sort agree with the oracle."""
    case = _case(box, pow2)
    parts = _lattice_particles(case, 700 + order)
    ws, srt = _sort(product, case, parts)
    a, s = np.array(parts), srt.to_numpy()
    assert np.array_equal(a[:, np.lexsort(a[::-1])], s[:, np.lexsort(s[::-1])])
    key, cell = H.tile_major_key(s[:3], case.plo, case.dinv, case.ncell)
    assert np.all(np.diff(key) >= 0)
    for d in range(3):   # the lower corner is in the first cell, the last double below the upper face in the last one
        assert cell[d][s[d] == case.plo[d]].size and not cell[d][s[d] == case.plo[d]].any()
        assert np.all(cell[d][s[d] == case.below_phi(d)] == case.ncell[d] - 1)
    ng = order + 2
    rho = case.field("rho", ng)
    rhod = rho.copy_to(DEV, True)
    ph = ParticleArrays.from_numpy(parts, "cpu")
    g = case.geom(ng)
    oracle.deposit_charge(C.byref(ph.view), C.byref(rho.view), C.byref(g), plasma.Q_E, order, None)
    product.deposit_charge(C.byref(srt.view), C.byref(rhod.view), C.byref(g), plasma.Q_E, order, None)
    product.device_synchronize()
    assert H.max_rel_err(rhod.to_numpy(), rho.to_numpy()) < 1e-12
    for algo in (ESIRKEPOV, DIRECT):
        _deposit_against_oracle(oracle, product, case, srt, ws, order, algo, 1e-12)
    for galerkin in (1, 0):
        ws2, srt2 = _sort(product, case, parts)
        _gather_against_oracle(oracle, product, case, srt2, ws2, order, galerkin)
        product.workspace_destroy(ws2)
    product.workspace_destroy(ws)


# ---- 3. particle counts around a wavefront, all in one tile ------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_particle_counts_in_one_tile(oracle, product, n, order):
    """1, 63, 64, 65 and 257 particles, all in the first tile of the offset box (the other three tiles are empty)."""
    case = _case("13x7x9_offset")
    parts = case.random_particles(n, 800 + n)
    rng = np.random.default_rng(n)
    for d in (0, 2):   # x and z have two tiles: keep to the first eight cells
        parts[d] = case.plo[d] + 8 * case.dx[d] * rng.random(n) * (1 - 1e-9)
    ws, srt = _sort(product, case, parts)
    key, _ = H.tile_major_key(srt.to_numpy()[:3], case.plo, case.dinv, case.ncell)
    assert np.all(key < 512)
    for algo in (ESIRKEPOV, DIRECT):
        _deposit_against_oracle(oracle, product, case, srt, ws, order, algo, 1e-12)
    for galerkin in (1, 0):
        ws2, srt2 = _sort(product, case, parts)
        _gather_against_oracle(oracle, product, case, srt2, ws2, order, galerkin)
        product.workspace_destroy(ws2)
    product.workspace_destroy(ws)


# ---- 4. the push in two parts ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("box,order,pusher", [("13x7x9_offset", 3, _capi.PUSHER_BORIS), ("13x7x9_offset", 2, _capi.PUSHER_VAY),
                                              ("17x24x25", 3, _capi.PUSHER_BORIS), ("17x24x25", 4, _capi.PUSHER_VAY)])
def test_gather_push_in_two_parts_on_odd_boxes(product, box, order, pusher):
    """wxa_gather_push_part, interior tiles then the rest, bit for bit one wxa_gather_push_ws call.  13 x 7 x 9: every tile
    touches a face, the interior part moves nothing.  17 x 24 x 25: 3 x 3 x 4 tiles, two interior ones, partial last tiles."""
    import torch
    case = _case(box)
    ng, _, _ = H.guard_depths(order)
    E = H.clone_fields(case.random_fields(("Ex", "Ey", "Ez"), ng, 10, scale=1e11), DEV, True)
    B = H.clone_fields(case.random_fields(("Bx", "By", "Bz"), ng, 11, scale=1e3), DEV, True)
    parts = case.random_particles(6000, 77)
    ntail = 200
    ws, full = _sort(product, case, parts, room=ntail)
    nsorted = full.np - ntail
    full.data[:, nsorted:] = torch.from_numpy(np.array(parts)[:, :ntail]).to(DEV)   # arrivals since the sort: anywhere
    start = full.data.clone()
    g = case.geom(ng)
    dt = H.yee_dt(case.dx)
    q, m = -plasma.Q_E, plasma.M_E
    product.gather_push_ws(C.byref(full.view), field_triplet(E), field_triplet(B), C.byref(g), q, m, dt, order, 1, pusher,
                           1, ws, None)
    product.device_synchronize()
    whole = full.data.clone()
    full.data.copy_(start)
    product.gather_push_part(C.byref(full.view), field_triplet(E), field_triplet(B), C.byref(g), q, m, dt, order, 1, pusher,
                             ws, _capi.PART_INTERIOR, None)
    product.device_synchronize()
    moved = (full.data[4] != start[4]).cpu().numpy() | (full.data[0] != start[0]).cpu().numpy()
    _, cell = H.tile_major_key(start[:3].cpu().numpy(), case.plo, case.dinv, case.ncell)
    face = np.zeros(full.np, dtype=bool)
    for d in range(3):
        nt = (case.ncell[d] + 7) // 8
        face |= (cell[d] // 8 == 0) | (cell[d] // 8 == nt - 1)
    assert not moved[nsorted:].any() and not (moved & face).any()
    assert moved[:nsorted][~face[:nsorted]].all()
    if box == "13x7x9_offset":
        assert face.all() and not moved.any()
    else:
        assert 0 < moved.sum() < nsorted
    product.gather_push_part(C.byref(full.view), field_triplet(E), field_triplet(B), C.byref(g), q, m, dt, order, 1, pusher,
                             ws, _capi.PART_REST, None)
    product.device_synchronize()
    assert torch.equal(full.data, whole)
    product.workspace_destroy(ws)


# ---- 5. the periodic wrap through the sort -------------------------------------------------------------------------------

@pytest.mark.parametrize("steps", [0, 3, 6])
def test_enforce_periodic_through_the_sort_on_an_odd_box(product, steps):
    """wxa_enforce_periodic_sorted against the plain pass, bit for bit, on 25 x 9 x 33 (4 x 2 x 5 tiles, one-cell last
    tiles in x and z: the tile before them is a face tile too) with the offset prob_lo, periodic in x and z."""
    import torch
    _, _, prob_lo, dx = BOXES["13x7x9_offset"]
    case = H.geom_case((25, 9, 33), (5, -3, 100), prob_lo, dx)
    n, ntail = 6000, 500
    ws, big = _sort(product, case, case.random_particles(n, 77), room=ntail)
    rng = np.random.default_rng(8)
    length = case.phi - case.plo
    for d in range(3):
        big.data[d][:n] += torch.from_numpy(case.dx[d] * max(steps, 0.5) * (2 * rng.random(n) - 1)).to(DEV)
        # the tail: anywhere within one period of the box
        big.data[d][n:] = torch.from_numpy(case.plo[d] + length[d] * (2.5 * rng.random(ntail) - 0.75)).to(DEV)
    ref = ParticleArrays(big.np, DEV)
    ref.data.copy_(big.data)
    before = big.to_numpy()
    per = (C.c_int * 3)(1, 0, 1)
    lo, hi = H.d3(case.plo), H.d3(case.phi)
    product.enforce_periodic(C.byref(ref.view), lo, hi, per, None)
    product.enforce_periodic_sorted(C.byref(big.view), lo, hi, per, ws, steps, None)
    product.device_synchronize()
    assert torch.equal(big.data, ref.data)
    a = ref.to_numpy()
    for d in (0, 2):
        assert np.all(a[d] >= case.plo[d]) and np.all(a[d] < case.phi[d])
        assert np.any(a[d, :n] != before[d, :n])            # some of the sorted ones did leave
    assert np.array_equal(a[1], before[1])
    product.workspace_destroy(ws)


# ---- 6. the sort folded into the push ----------------------------------------------------------------------------------

@pytest.mark.parametrize("order,predict", [(3, True), (2, False)])
def test_sort_folded_into_the_push_on_the_offset_box(oracle, product, order, predict):
    """One cycle of wxa_push_sort_begin / _end on the offset 13 x 7 x 9 box: a push that records keys and ranks (COUNT), a
    push that writes the particles into the sorted tile (SCATTER), a push on that tile through the workspace the SCATTER
    left.  Every particle arrives with its own data (ids), pushed as the oracle pushes it; the new order is the tile-major
    cell order of the positions the COUNT keyed (carried one step further in free flight with predict_dt), wrapped along
    the periodic directions."""
    import torch
    case = _case("13x7x9_offset")
    ng, _, _ = H.guard_depths(order)
    E = case.random_fields(("Ex", "Ey", "Ez"), ng, 10, scale=1e11)
    B = case.random_fields(("Bx", "By", "Bz"), ng, 11, scale=1e3)
    Ed, Bd = H.clone_fields(E, DEV, True), H.clone_fields(B, DEV, True)
    n = 6000
    parts = case.random_particles(n, 500 + order, u_scale=30.0)   # up to ~0.5 cell per push
    wrap_flags = (1, 0, 1)
    wrap = (C.c_int32 * 3)(*wrap_flags)
    plo, dinv, lo, nc = case.sort_args()
    g = case.geom(ng)
    dt = H.yee_dt(case.dx)
    q, m = -plasma.Q_E, plasma.M_E
    ids = np.arange(1, n + 1, dtype=np.int64)
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    src = ParticleArrays.from_numpy(parts, DEV, ids)
    cur = ParticleArrays(n, DEV, with_id=True)
    product.sort_particles_by_cell(C.byref(src.view), C.byref(cur.view), plo, dinv, lo, nc, ws, None)
    product.device_synchronize()
    spare = ParticleArrays(n, DEV, with_id=True)
    length = case.phi - case.plo

    def keep_inside(pa):   # what Redistribute does between two pushes: periodic wrap, or a wall that keeps them in
        for d in range(3):
            x = pa.data[d]
            if wrap_flags[d]:
                x.copy_(torch.where(x >= case.phi[d], x - length[d], torch.where(x < case.plo[d], x + length[d], x)))
            x.clamp_(float(case.plo[d]), float(case.below_phi(d)))

    def oracle_push(rows):
        ph = ParticleArrays.from_numpy(list(rows), "cpu")
        oracle.gather_push(C.byref(ph.view), field_triplet(E), field_triplet(B), C.byref(g), q, m, dt, order, 1,
                           _capi.PUSHER_BORIS, None)
        return ph.to_numpy()

    live, appended = C.c_int64(), C.c_int64()
    key_of = key_ids = None
    for mode in (_capi.PUSH_SORT_COUNT, _capi.PUSH_SORT_SCATTER, 0):
        before, before_ids = cur.to_numpy(), cur.ids_to_numpy()
        want = oracle_push(before)
        if mode:
            assert (product.push_sort_pending(ws, C.byref(cur.view)) == 1) == (mode == _capi.PUSH_SORT_SCATTER)
            product.push_sort_begin(ws, mode, C.byref(cur.view), C.byref(spare.view), plo, dinv, lo, nc, wrap, 0,
                                    dt if predict else 0.0, None)
        product.gather_push_ws(C.byref(cur.view), field_triplet(Ed), field_triplet(Bd), C.byref(g), q, m, dt, order, 1,
                               _capi.PUSHER_BORIS, 1, ws, None)
        if mode:
            product.push_sort_end(ws, 0, C.byref(live), C.byref(appended), None)
        product.device_synchronize()
        if mode == _capi.PUSH_SORT_SCATTER:
            assert live.value == n and appended.value == 0
            got, got_ids = spare.to_numpy(), spare.ids_to_numpy()
            ow, og = np.argsort(before_ids), np.argsort(got_ids)
            assert np.array_equal(before_ids[ow], got_ids[og])
            for row in range(7):
                assert H.max_rel_err(got[row][og], want[row][ow]) < 1e-12, row
            id_to_key = dict(zip(key_ids.tolist(), key_of.tolist()))
            assert np.all(np.diff(np.array([id_to_key[i] for i in got_ids.tolist()])) >= 0)
            cur, spare = spare, cur
        else:
            got = cur.to_numpy()
            assert np.array_equal(cur.ids_to_numpy(), before_ids)
            for row in range(7):
                assert H.max_rel_err(got[row], want[row]) < 1e-12, row
        if mode == _capi.PUSH_SORT_COUNT:   # what the record should hold: keys of the positions this push produced
            after = cur.to_numpy()
            where = after[:3]
            if predict:
                gam = np.sqrt(1.0 + (after[4] ** 2 + after[5] ** 2 + after[6] ** 2) / plasma.C_LIGHT ** 2)
                where = [after[d] + after[4 + d] / gam * dt for d in range(3)]
            key_of, _ = H.tile_major_key(where, case.plo, case.dinv, case.ncell, wrap_flags)
            key_ids = cur.ids_to_numpy()
        keep_inside(cur)
    product.workspace_destroy(ws)


# ---- 7. the HIP kernels against the definitions ------------------------------------------------------------------------

@pytest.mark.parametrize("op", M.OPS)
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_hip_kernels_against_the_model(product, op, order):
    """The global kernels and the LDS-tile kernels against tests/spline_model.py, 300 particles in the offset box, at the
    gates of the oracle against the model (ten times the oracle's own figure, at most the parity gate)."""
    case = _case("13x7x9_offset")
    parts = M.case_particles(case, op, 300, 100 * order + len(op), lattice=False)
    errs = {"global": M.library_error(product, DEV, op, order, case, parts)}
    if op != "charge":
        errs["tiles"] = M.library_error(product, DEV, op, order, case, parts, tiles=True)
    print(f"HIP vs model {op} order {order}: {errs} (gate {M.gate(op, order):.1e})")
    assert max(errs.values()) < M.gate(op, order), errs
