"""The momentum push of the HIP kernels against tests/pusher_model.py, per particle and per regime.

push_boris, push_vay, push_hc, push_boris_rr and update_position (csrc/shapes.hpp) are inlined into three kernels: the
global-memory gather, the LDS-tile gather and its straggler pass.  The parity tests hold them to the oracle under a
max-norm at |u| ~ c with a rotation angle of 1e-5; here every kernel's copy runs the grid of tests/test_pusher_model_cpu.py
(u/c from 1e-8 to 1e4, field-free to |q| B dt / 2m ~ 8e3, E parallel and perpendicular to B, three species) against the
long-double model, with the gate table that the oracle's own error sets (pusher_model.GATES).  The grid fields are exact
zeros and E, B are the container's constant external fields, so the pushers see them exactly."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from tests import pusher_model as M
from warpx_amd import _capi
from warpx_amd.containers import ParticleArrays, field_triplet

pytestmark = pytest.mark.gpu

DEV = H.DEVICE
# route: (order, sorted).  Unsorted particles take the global-memory kernel, sorted ones the LDS tiles.
ROUTES = {"global_order1": (1, False), "tiles_order3": (3, True)}
_fields = {}


def _zero_fields(order):
    if order not in _fields:
        E, B, g = M.zero_fields(order)
        _fields[order] = (H.clone_fields(E, DEV, True), H.clone_fields(B, DEV, True), g)
    return _fields[order]


def _stragglers(product, ws):
    n = C.c_int64(-1)
    product.workspace_last_stragglers(ws, _capi.TILE_GATHER, C.byref(n))
    return n.value


def product_push(product, ws, route, pusher, parts, E, B, q, m, dt, move, leave_tile=None):
    """PushP / PushPX of the product through wxa_gather_push_ws; returns the particle rows in the order of `parts`, the
    positions the kernel was handed, and how many particles the tile kernel left to its straggler pass (None on the
    global route).  leave_tile: a mask over `parts` of particles that are put 1.5 cells below the box in x behind the
    sort: their stencils leave the staged tile, inside the guard cells of the fields."""
    order, sort = ROUTES[route]
    Ed, Bd, g = _zero_fields(order)
    n = len(parts[0])
    product.workspace_set_external_particle_fields(ws, H.d3(E), H.d3(B))
    pd = ParticleArrays.from_numpy(parts, DEV, np.arange(1, n + 1, dtype=np.int64))
    x_in = np.array(parts[0:3])
    if sort:
        srt = ParticleArrays(n, DEV, with_id=True)
        dx = H.LX / np.asarray(M.NCELL)
        product.sort_particles_by_cell(C.byref(pd.view), C.byref(srt.view), H.d3((-H.LX / 2,) * 3), H.d3(1.0 / dx),
                                       (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*M.NCELL), ws, None)
        product.device_synchronize()
        pd = srt
        if leave_tile is not None:
            import torch
            where = pd.ids_to_numpy().astype(np.int64) - 1
            x_in[0, leave_tile] = -H.LX / 2 - 1.5 * dx[0]
            pd.data[0].copy_(torch.from_numpy(x_in[0, where]).to(DEV))
    product.gather_push_ws(C.byref(pd.view), field_triplet(Ed), field_triplet(Bd), C.byref(g), q, m, dt, order, 1,
                           M.PUSHERS[pusher][1], move, ws, None)
    product.device_synchronize()
    handed_on = _stragglers(product, ws) if sort else None
    got = pd.to_numpy()
    rows = np.empty_like(got)
    rows[:, pd.ids_to_numpy().astype(np.int64) - 1] = got
    return rows, x_in, handed_on


def _bound(oracle, pusher, fields, species, u_over_c):
    """The cell's gate; in a reported cell four times the oracle's own worst error there (never below 16)."""
    if (pusher, fields) not in M.REPORTED:
        return M.gate(pusher, fields, u_over_c)
    parts, E, B, q, m, dt, _ = M.launch_inputs(fields, species, u_over_c)
    err, _ = M.judge(M.oracle_push(oracle, pusher, parts, E, B, q, m, dt, 0), pusher, fields, species, u_over_c, 0, 0)
    return max(16.0, 4.0 * float(err.max()))


def _run_cells(oracle, product, route, pusher, fields, cells, move, leave_tile=None):
    """Every (species, u/c) of `cells` through the product; returns the lines of the cells that failed, worst first."""
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    failed = []
    for species, u_over_c in cells:
        parts, E, B, q, m, dt, names = M.launch_inputs(fields, species, u_over_c)
        mask = None if leave_tile is None else leave_tile(len(parts[0]))
        got, x_in, handed_on = product_push(product, ws, route, pusher, parts, E, B, q, m, dt, move, mask)
        assert np.all(np.isfinite(got)), (pusher, fields, species, u_over_c)
        if handed_on is not None:
            assert handed_on == (0 if mask is None else int(mask.sum())), handed_on
        if fields == "none":
            assert names[0] == "u=0" and not np.any(got[4:7, 0])      # exactly zero
        bound = _bound(oracle, pusher, fields, species, u_over_c)
        parts_seen = [x_in[0], x_in[1], x_in[2]] + list(parts[3:])
        err, excess = M.judge(got, pusher, fields, species, u_over_c, move, bound, parts=parts_seen)
        print(f"{route} {pusher} {fields} {species} u/c={u_over_c:g} move={move}: {err.max():.1f} ulp (bound {bound:g})"
              + (f", position {excess.max():.3f} of its bound" if move else ""))
        if err.max() > bound:
            failed.append((float(err.max() / bound), M.describe(got, pusher, fields, species, u_over_c, err) + f" bound {bound:g}"))
        if excess.max() > 1.0:
            i = int(np.argmax(excess))
            failed.append((float(excess.max()), f"{pusher} {fields} {species} u/c={u_over_c:g}: position of particle {i} "
                           f"{excess[i]:.2f} of its bound, x_in={x_in[:, i].tolist()} got={got[0:3, i].tolist()}"))
    product.workspace_destroy(ws)
    return [line for _, line in sorted(failed, reverse=True)]


ALL_CELLS = [(species, u) for species in M.SPECIES for u in M.U_OVER_C]


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("pusher", list(M.PUSHERS))
@pytest.mark.parametrize("fields", M.ALL_FIELD_SETS)
def test_push_against_the_model(oracle, product, route, pusher, fields):
    """PushP (move 0) on 4096 particles per launch, three species and five u/c per case, on the global-memory kernel
    (order 1, unsorted) and on the LDS tiles (order 3, behind the cell sort, nothing handed to the straggler pass)."""
    failed = _run_cells(oracle, product, route, pusher, fields, ALL_CELLS, 0)
    assert not failed, f"{len(failed)} cells, worst first:\n" + "\n".join(failed[:3])


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("pusher", list(M.PUSHERS))
@pytest.mark.parametrize("fields", M.MOVE_FIELD_SETS)
def test_position_update_against_the_model(oracle, product, route, pusher, fields):
    """PushPX (move 1): the same momenta, and x + v(u_new) dt within one ulp of the box's largest coordinate plus the
    cell's gate on the displacement."""
    failed = _run_cells(oracle, product, route, pusher, fields, [("electron", u) for u in M.MOVE_U_OVER_C], 1)
    assert not failed, f"{len(failed)} cells, worst first:\n" + "\n".join(failed[:3])


@pytest.mark.parametrize("pusher", list(M.PUSHERS))
@pytest.mark.parametrize("move", [0, 1])
def test_push_in_the_straggler_kernel(oracle, product, pusher, move):
    """The straggler pass has its own copy of the pusher: every seventh particle and the exact-input rows sit 1.5 cells
    below the box behind the sort, so the tile kernel hands exactly them on (the count is asserted in _run_cells)."""
    def leave_tile(n):
        mask = np.arange(n) % 7 == 0
        mask[:8] = True
        return mask
    for fields in ("rr_regime", "B_tau4"):
        failed = _run_cells(oracle, product, "tiles_order3", pusher, fields, [("electron", 1.0), ("proton", 1e4)], move, leave_tile)
        assert not failed, f"{len(failed)} cells, worst first:\n" + "\n".join(failed[:3])
