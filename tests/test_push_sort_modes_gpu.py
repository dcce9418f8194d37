"""The cell sort folded into PushPX in each of its modes and through each PART launch (csrc/push_sort.hpp, gather_tile.hip).

Three pushes of a classically sorted tile: COUNT, then SCATTER (or, with `every_step`, COUNT | SCATTER and a closing
SCATTER), through `wxa_gather_push_ws` (every tile in one launch) or the two `wxa_gather_push_part` launches.  Checked on
the host, from what is downloaded:
  * momenta and positions of every push equal those of the PLAIN push of the same tile bit for bit (the plain push runs
    first, in place, on the same arrays with the same workspace; the arrays are then put back), after undoing the
    permutation by the ids;
  * the sorted tile is the counting sort of the record's keys -- the tile-major `cell_of` of the positions the counting push
    produced (no prediction: the keys are then exactly computable) -- ties in any order: every counted live particle
    exactly once (so the scanned offsets and the ranks tile the range without gap or overlap), keys non-decreasing,
    retired ones dropped, appended ones behind in their order; live / appended counts as computed on the host.
Every case asserts that its inputs contain what it is named after."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from warpx_amd import _capi, plasma
from warpx_amd.containers import ParticleArrays, field_triplet

pytestmark = pytest.mark.gpu

DEV = H.DEVICE
NCELL = (32, 24, 24)   # 4 x 3 x 3 tiles of 8^3 cells: two of them (16, 17) touch no face
NTILES = 36
TILE_CELLS = 512


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


@pytest.mark.parametrize("every_step", [False, True], ids=["count_then_scatter", "count_and_scatter"])
@pytest.mark.parametrize("parts", [False, True], ids=["all_tiles", "interior_and_rest"])
@pytest.mark.parametrize("case", ["retired_appended", "empty_tile", "heavy_tile", "stale_sort"])
def test_push_sort_modes(product, case, parts, every_step, monkeypatch):
    import torch
    order = 3
    if case == "heavy_tile":
        monkeypatch.setenv("WXA_HEAVY_TILE", "400")
    ng, _, _ = H.guard_depths(order)
    E = H.random_fields(("Ex", "Ey", "Ez"), NCELL, ng, 10, scale=1e11)
    B = H.random_fields(("Bx", "By", "Bz"), NCELL, ng, 11, scale=1e3)
    Ed, Bd = H.clone_fields(E, DEV, True), H.clone_fields(B, DEV, True)
    dx = H.LX / np.asarray(NCELL)
    plo, dinv = H.d3((-H.LX / 2,) * 3), H.d3(1.0 / dx)
    lo, nc = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*NCELL)
    wrap_flags = (1, 0, 1)
    wrap = (C.c_int32 * 3)(*wrap_flags)
    g, _ = H.geom_for(NCELL, ng)
    dt = H.yee_dt(dx)
    q, m = -plasma.Q_E, plasma.M_E
    n0, n_tail, n_arrive = 20000, 300, 200
    # up to ~0.5 cell per push; the stale sort moves them further, so that a good part leaves its tile between two sorts
    rows = [np.asarray(r) for r in H.random_particles(n0, NCELL, 77, u_scale=90.0 if case == "stale_sort" else 30.0)]
    key0 = _tile_major_key(rows[:3], NCELL, dx, wrap_flags)
    if case == "empty_tile":   # nobody in tile 17, one of the two interior ones
        keep = key0 // TILE_CELLS != 17
        rows = [r[keep] for r in rows]
        n0 = int(keep.sum())
        per_tile = np.bincount(_tile_major_key(rows[:3], NCELL, dx, wrap_flags) // TILE_CELLS, minlength=NTILES)
        assert per_tile[17] == 0 and per_tile[16] > 0, per_tile
    if case == "heavy_tile":
        per_tile = np.bincount(key0 // TILE_CELLS, minlength=NTILES)
        assert per_tile.max() > 400, per_tile   # shared by several workgroups
    with_tail = case == "retired_appended"
    tail = [np.asarray(r) for r in H.random_particles(n_tail, NCELL, 78, u_scale=30.0)] if with_tail else None
    cap = n0 + n_tail + n_arrive
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    cur, spare = ParticleArrays(cap, DEV, with_id=True), ParticleArrays(cap, DEV, with_id=True)
    src = ParticleArrays.from_numpy(rows, DEV, np.arange(1, n0 + 1, dtype=np.int64))

    def view_of(pa, n):
        v = pa.view
        v.np = n
        return v

    v = view_of(cur, n0)
    product.sort_particles_by_cell(C.byref(src.view), C.byref(v), plo, dinv, lo, nc, ws, None)
    product.device_synchronize()
    npart = n0
    if with_tail:   # appended behind the sorted part before the COUNT: the global-memory kernel's particles
        for r in range(7):
            cur.data[r][n0:n0 + n_tail] = torch.from_numpy(tail[r]).to(DEV)
        cur.idcpu[n0:n0 + n_tail] = torch.from_numpy(np.arange(10 ** 5, 10 ** 5 + n_tail, dtype=np.int64)).to(DEV)
        npart += n_tail

    def host_copy(pa, n):
        return pa.to_numpy()[:, :n].copy(), pa.ids_to_numpy()[:n].copy()

    def push(pa, n):
        pv = view_of(pa, n)
        args = (field_triplet(Ed), field_triplet(Bd), C.byref(g), q, m, dt, order, 1, _capi.PUSHER_BORIS)
        if parts:
            product.gather_push_part(C.byref(pv), *args, ws, _capi.PART_INTERIOR, None)
            product.gather_push_part(C.byref(pv), *args, ws, _capi.PART_REST, None)
        else:
            product.gather_push_ws(C.byref(pv), *args, 1, ws, None)
        product.device_synchronize()

    def keep_inside(pa, n):   # Redistribute between two pushes: periodic wrap, or a wall
        for d in range(3):
            x = pa.data[d][:n]
            if wrap_flags[d]:
                x.copy_(torch.where(x >= H.LX / 2, x - H.LX, torch.where(x < -H.LX / 2, x + H.LX, x)))
            else:
                x.clamp_(-H.LX / 2, H.LX / 2 - 1e-12)

    C_, S_ = _capi.PUSH_SORT_COUNT, _capi.PUSH_SORT_SCATTER
    modes = [C_, C_ | S_, S_] if every_step else [C_, S_]

    def tiles_of(pos):
        return _tile_major_key(pos, NCELL, dx, wrap_flags) // TILE_CELLS

    slot_tile = tiles_of(host_copy(cur, n0)[0][:3])   # tile whose workgroup pushes slot i of the sorted part (-1: unknown)
    n_sorted = n0                                     # particles the tile kernel pushes
    live_i64, app_i64 = C.c_int64(), C.c_int64()
    record = None          # (keys, n_counted, retired slots) of the pending COUNT, indexed by slot
    seen = {"foreign": 0, "straggler": 0, "retired": 0, "appended": 0}
    for step, mode in enumerate(modes):
        before, before_ids = host_copy(cur, npart)
        known = slot_tile[:n_sorted] >= 0
        # stragglers of this push: sorted particles that are no longer in the tile they were sorted into
        seen["straggler"] += int((tiles_of(before[:3])[:n_sorted] != slot_tile[:n_sorted])[known].sum())
        seen["retired"] += int((before_ids == -1).sum())
        # the plain push of the same tile, in place; then the arrays as they were
        saved = [cur.data[r][:npart].clone() for r in range(7)]
        push(cur, npart)
        plain, plain_ids = host_copy(cur, npart)
        assert np.array_equal(plain_ids, before_ids)
        for r in range(7):
            cur.data[r][:npart].copy_(saved[r])
        if mode & C_:   # foreign: keyed into a tile other than the counting workgroup's, or counted by the global-memory kernel
            seen["foreign"] += int((tiles_of(plain[:3])[:n_sorted] != slot_tile[:n_sorted])[known].sum()) + (npart - n_sorted)
        pv, dv = view_of(cur, npart), view_of(spare, npart)
        assert (product.push_sort_pending(ws, C.byref(pv)) == 1) == bool(mode & S_)
        rc = product.push_sort_begin(ws, mode, C.byref(pv), C.byref(dv), plo, dinv, lo, nc, wrap, 1, 0.0, None)
        assert rc == 0, product.last_error()
        push(cur, npart)
        n_retired_rec = len(record[2]) if record else 0
        rc = product.push_sort_end(ws, 1 if (mode & S_) and n_retired_rec else 0, C.byref(live_i64), C.byref(app_i64), None)
        assert rc == 0, product.last_error()
        product.device_synchronize()
        if mode & S_:
            rec_keys, n_counted, rec_retired = record
            live, appended = live_i64.value, app_i64.value
            assert live == n_counted - len(rec_retired) and appended == npart - n_counted
            seen["appended"] += appended
            got, got_ids = host_copy(spare, live + appended)
            # the cell-sorted part: the record's surviving slots, each exactly once, by non-decreasing key; the particles
            # retired SINCE the count keep the slot they were counted into (id -1), those of the record are dropped
            surviving = np.ones(n_counted, bool)
            surviving[rec_retired] = False
            want_ids = before_ids[:n_counted][surviving]
            live_ids = got_ids[:live]
            assert np.array_equal(np.sort(live_ids), np.sort(want_ids))
            assert len(np.unique(live_ids[live_ids != -1])) == (live_ids != -1).sum()
            key_by_id = dict(zip(before_ids[:n_counted].tolist(), rec_keys.tolist()))
            keys_sorted = np.array([key_by_id[i] for i in live_ids.tolist() if i != -1])
            assert np.all(np.diff(keys_sorted) >= 0)
            # the arrivals behind it in their order
            assert np.array_equal(got_ids[live:], before_ids[n_counted:])
            # bit for bit the plain push, after undoing the permutation
            lw = before_ids != -1
            lg = got_ids != -1
            ow, og = np.argsort(before_ids[lw]), np.argsort(got_ids[lg])
            assert np.array_equal(before_ids[lw][ow], got_ids[lg][og])
            for r in range(7):
                assert np.array_equal(got[r][lg][og], plain[r][lw][ow]), (step, r)
            assert np.all(got[3][got_ids == -1] == 0.0)
            cur, spare = spare, cur
            npart = live + appended
            n_sorted = live
            slot_tile = np.array([key_by_id[i] // TILE_CELLS if i != -1 else -1 for i in live_ids.tolist()])
        else:
            got, got_ids = host_copy(cur, npart)
            assert np.array_equal(got_ids, before_ids)
            for r in range(7):
                assert np.array_equal(got[r], plain[r]), (step, r)
        if mode & C_:   # what the record holds: keys of the positions this push produced, retired ones in the last bin
            record = (_tile_major_key(got[:3], NCELL, dx, wrap_flags), npart, np.nonzero(got_ids == -1)[0])
        else:
            record = None
        keep_inside(cur, npart)
        if step == 0 and case == "retired_appended":
            rng = np.random.default_rng(5)
            gone = torch.from_numpy(rng.random(npart) < 0.01).to(DEV)   # retired after the COUNT: they keep their slot ...
            cur.idcpu[:npart][gone] = -1
            cur.data[3][:npart][gone] = 0.0
            arr = [np.asarray(r) for r in H.random_particles(n_arrive, NCELL, 900, u_scale=30.0)]   # ... and arrivals
            for r in range(7):
                cur.data[r][npart:npart + n_arrive] = torch.from_numpy(arr[r]).to(DEV)
            cur.idcpu[npart:npart + n_arrive] = torch.from_numpy(np.arange(10 ** 6, 10 ** 6 + n_arrive, dtype=np.int64)).to(DEV)
            npart += n_arrive
    product.workspace_destroy(ws)
    # the inputs held what the case is named after
    assert seen["foreign"] >= 1 and seen["straggler"] >= 1, seen
    if case == "retired_appended":
        assert seen["appended"] >= 1 and seen["retired"] >= 1, seen
    if case == "stale_sort":
        assert seen["straggler"] >= n0 // 20, seen


def test_push_sort_protocol(product):
    """The record of a COUNT through its life (include/warpx_amd.h, wxa_push_sort_begin): who it is pending for, what
    drops it, every refused begin / end, and that a refused call arms nothing and drops nothing -- a correct
    begin / push / end follows each one on the same workspace.  (16, 8, 8) cells: two tiles; 2 000 sorted particles and
    50 appended behind them; order 1.  No tolerance: statuses, the pending flag, and one bit-for-bit comparison."""
    import torch
    ncell, order = (16, 8, 8), 1
    n0, n_tail = 2000, 50
    npart = n0 + n_tail
    ng, _, _ = H.guard_depths(order)
    Ed = H.clone_fields(H.random_fields(("Ex", "Ey", "Ez"), ncell, ng, 10, scale=1e11), DEV, True)
    Bd = H.clone_fields(H.random_fields(("Bx", "By", "Bz"), ncell, ng, 11, scale=1e3), DEV, True)
    g, dx = H.geom_for(ncell, ng)
    dt = H.yee_dt(dx)
    q, m = -plasma.Q_E, plasma.M_E
    plo, phi, dinv = H.d3((-H.LX / 2,) * 3), H.d3((H.LX / 2,) * 3), H.d3(1.0 / dx)
    lo, nc, wrap = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*ncell), (C.c_int32 * 3)(1, 1, 1)
    per = H.i3((1, 1, 1))
    rows = [np.asarray(r) for r in H.random_particles(n0, ncell, 77, u_scale=30.0)]
    tail = [np.asarray(r) for r in H.random_particles(n_tail, ncell, 78, u_scale=30.0)]
    src = ParticleArrays.from_numpy(rows, DEV, np.arange(1, n0 + 1, dtype=np.int64))
    cap = npart + 8
    a, b, other = (ParticleArrays(cap, DEV, with_id=True) for _ in range(3))
    ws = C.c_void_p()
    product.workspace_create(C.byref(ws))
    C_, S_ = _capi.PUSH_SORT_COUNT, _capi.PUSH_SORT_SCATTER
    live, app = C.c_int64(), C.c_int64()

    def view_of(pa, n):
        v = pa.view
        v.np = n
        return v

    def pending(pa, n=npart):
        return product.push_sort_pending(ws, C.byref(view_of(pa, n)))

    def sort_into_a():   # the classic sort: a's first n0 particles are src in cell order, the tail stays behind them
        product.sort_particles_by_cell(C.byref(src.view), C.byref(view_of(a, n0)), plo, dinv, lo, nc, ws, None)
        product.device_synchronize()

    def begin(mode, p, d, np_=npart, nd=npart):
        product.push_sort_begin(ws, mode, C.byref(view_of(p, np_)), C.byref(view_of(d, nd)), plo, dinv, lo, nc, wrap, 0, 0.0, None)

    def push_and_end(p):
        pv = view_of(p, npart)
        product.gather_push_ws(C.byref(pv), field_triplet(Ed), field_triplet(Bd), C.byref(g), q, m, dt, order, 1,
                               _capi.PUSHER_BORIS, 1, ws, None)
        product.push_sort_end(ws, 0, C.byref(live), C.byref(app), None)
        product.enforce_periodic(C.byref(pv), plo, phi, per, None)   # Redistribute: nobody drifts out of the guard cells
        product.device_synchronize()

    def take_record():   # a correct begin / push / end
        begin(C_, a, b)
        push_and_end(a)
        assert pending(a) == 1

    sort_into_a()
    assert pending(a) == 0
    for r in range(7):
        a.data[r][n0:npart] = torch.from_numpy(tail[r]).to(DEV)
    a.idcpu[n0:npart] = torch.from_numpy(np.arange(10 ** 5, 10 ** 5 + n_tail, dtype=np.int64)).to(DEV)

    # who the record is pending for
    take_record()
    assert live.value == npart and app.value == 0
    assert pending(other) == 0
    assert pending(a, npart - 1) == 0 and pending(a, npart + 1) == 1
    # what drops it
    sort_into_a()
    assert pending(a) == 0
    take_record()
    counts = (C.c_int64 * 3)()
    product.partition_particles(C.byref(src.view), C.byref(view_of(b, n0)), 0, -H.LX / 4, H.LX / 4, counts, ws, None)
    assert sum(counts) == n0 and pending(a) == 0
    sort_into_a()   # (the partition dropped the tiles as well)

    # begin while armed
    begin(C_, a, b)
    with pytest.raises(_capi.WxaError, match="without the wxa_push_sort_end"):
        begin(C_, a, b)
    push_and_end(a)   # still armed, by the first begin only
    assert pending(a) == 1
    take_record()
    # end with nothing armed
    with pytest.raises(_capi.WxaError, match="without wxa_push_sort_begin"):
        product.push_sort_end(ws, 0, C.byref(live), C.byref(app), None)
    take_record()
    # SCATTER with no record
    sort_into_a()
    assert pending(a) == 0
    with pytest.raises(_capi.WxaError, match="no record of a COUNT"):
        begin(S_, a, b)
    take_record()
    # SCATTER with a record on other arrays, with dst aliasing p, with dst shorter than p: the record stays pending
    for p, d, nd in ((other, b, npart), (a, a, npart), (a, b, npart - 1)):
        with pytest.raises(_capi.WxaError):
            begin(S_, p, d, nd=nd)
        assert pending(a) == 1
        with pytest.raises(_capi.WxaError, match="without wxa_push_sort_begin"):   # nothing was armed
            product.push_sort_end(ws, 0, C.byref(live), C.byref(app), None)
        take_record()
    # the record is still good for what it is for: the sorting push into b, which takes the next record with it
    begin(C_ | S_, a, b)
    push_and_end(a)
    assert live.value + app.value == npart
    assert pending(b) == 1 and pending(a) == 0

    # no sort recorded: nothing to count
    ws2 = C.c_void_p()
    product.workspace_create(C.byref(ws2))
    with pytest.raises(_capi.WxaError, match="no sort recorded"):
        product.sort_live_count(ws2, C.byref(live), None)
    product.workspace_destroy(ws2)
    # the sort in ws is of b: on another array the wrap through the sort is the plain pass, bit for bit
    rng = np.random.default_rng(8)
    for d in range(3):
        other.data[d][:npart] = torch.from_numpy(H.LX * (1.5 * rng.random(npart) - 0.75)).to(DEV)
    ref = ParticleArrays(cap, DEV, with_id=True)
    ref.data.copy_(other.data)
    product.enforce_periodic(C.byref(view_of(ref, npart)), plo, phi, per, None)
    product.enforce_periodic_sorted(C.byref(view_of(other, npart)), plo, phi, per, ws, 0, None)
    product.device_synchronize()
    assert torch.equal(other.data[:3, :npart], ref.data[:3, :npart])
    got = other.data[:3, :npart]
    assert bool(((got >= -H.LX / 2) & (got < H.LX / 2)).all())
    product.workspace_destroy(ws)
