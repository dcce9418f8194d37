"""tests/decks/density_ramp_window_3d.inputs on the HIP path: <species>.profile = parse_density_function behind a moving
window.  The plasma is at rest and there is no laser, so J stays zero and nothing moves: after the run the particles are
the numpy model's (tests/plasma_profile_model.py), bit for bit in position and weight -- every particle on the injection
lattice with w = n(x, y, z) dV / nppc of its own position, and as many as the final window's cells emit.  The same deck
on two bricks in x (threads of this process over ThreadBrickTransport) gives the same set: each brick injects the cells
of its own overlap through its own workspace, programs and probe mask."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

from tests import plasma_profile_model as M
from tests.test_multibrick_gpu import ThreadBrickTransport, thread_transport_abort, thread_transport_state
from warpx_amd import _capi
from warpx_amd.distributed import brick_coord
from warpx_amd.sim import WarpXSim

pytestmark = pytest.mark.gpu

DECKS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "decks")
DECK = os.path.join(DECKS, "density_ramp_window_3d.inputs")


def test_ramp_deck_ends_with_the_models_particles(product):
    sim = WarpXSim.from_inputs(product, DECK)
    assert sim.max_step == 48
    sim.evolve(sim.max_step)
    got = M.sort_by_position(sim.particles(0))
    want, shifts = M.ramp_deck_particles(sim.istep * sim.dt)
    assert shifts > 32          # every particle of the final window came in through continuous injection
    assert want.shape[1] > 10000
    for name in ("jx", "jy", "jz"):
        assert not sim.field(name).any()
    assert got.shape[1] == want.shape[1]
    assert np.array_equal(got[:3], want[:3])
    assert np.array_equal(got[3], want[3])
    assert np.all(got[4:] == 0.0)
    # the weight is the density at the particle's own position (the model's statement, spelled out)
    dv = M.UM * M.UM * (M.UM / 2)
    assert np.array_equal(got[3], M.ramp_deck_density(got[0], got[1], got[2]) * (dv / 2))
    sim.close()


def run_deck_on_bricks(product, nb):
    """the deck's run cut into nb bricks; every brick's particles and the time reached"""
    nranks = nb[0] * nb[1] * nb[2]
    shared = thread_transport_state()
    results, errors = [None] * nranks, []

    def brick(rank):
        shared["turn"].acquire()
        try:
            tr = ThreadBrickTransport(rank, nranks, shared)
            sim = WarpXSim.from_inputs(product, DECK, nbricks=nb, coord=brick_coord(rank, nb), comm=tr.comm)
            sim.evolve(sim.max_step)
            results[rank] = {"particles": sim.particles(0), "t": sim.istep * sim.dt}
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
    return results


def test_two_bricks_in_x_end_with_the_one_bricks_particles(product):
    results = run_deck_on_bricks(product, (2, 1, 1))
    left, right = (r["particles"] for r in results)
    assert left.shape[1] > 5000 and right.shape[1] > 5000
    assert np.all(left[0] < 0.0) and np.all(right[0] > 0.0)   # the bricks meet at x = 0
    two = M.sort_by_position(np.concatenate([left, right], axis=1))
    sim = WarpXSim.from_inputs(product, DECK)
    sim.evolve(sim.max_step)
    one = M.sort_by_position(sim.particles(0))
    sim.close()
    want, _ = M.ramp_deck_particles(results[0]["t"])
    assert two.shape == one.shape == want.shape
    assert np.array_equal(two, one) and np.array_equal(two[:4], want[:4])


def test_injection_profile_without_a_deck(product):
    """WarpXSim.set_injection_profile (wxa_sim_set_injection_profile): add_initial fills the domain now, from compiled
    expressions; 8 x 8 x 8 cells, the ramp starts inside the box"""
    n, length = 8, 8 * M.UM
    sim = WarpXSim(product, (n, n, n), (0.0, 0.0, 0.0), (length, length, length), nox=1)
    empty, sid = _capi.ParticleView(), C.c_int32()
    product.sim_add_species(sim._h, -1.602176634e-19, 9.1093837015e-31, C.byref(empty), C.byref(sid))
    consts = {"n0": 2.e23, "zs": 2 * M.UM, "L": 24 * M.UM, "rc": 10 * M.UM}
    dens = _capi.Expr(product, "n0*(z-zs)/L*(1+4*(x*x+y*y)/(rc*rc))*(z>=zs)", constants=consts)
    inj = _capi.PlasmaInjector()
    for d in range(3):
        inj.ppc[d] = (2, 1, 2)[d]
        inj.lo[d], inj.hi[d] = -M.FLT_MAX, M.FLT_MAX
    dmin, dmax = 0.05 * 2.e23, 0.2 * 2.e23
    sim.set_injection_profile(sid.value, inj, dens, density_min=dmin, density_max=dmax, add_initial=True, continuous=False)
    got = M.sort_by_position(sim.particles(sid.value))
    want, raw = M.add_plasma(M.ramp_deck_density, corner=(0.0, 0.0, 0.0), ncells=(n, n, n), dx=(M.UM,) * 3, ppc=(2, 1, 2),
                             lo=(-M.FLT_MAX,) * 3, hi=(M.FLT_MAX,) * 3, brick_lo=(0.0,) * 3, brick_hi=(length,) * 3,
                             density_min=dmin, density_max=dmax)
    for thr in (dmin, dmax):
        assert np.min(np.abs(raw - thr)) > 1e-9 * thr
    assert 0 < want.shape[1] < n * n * n * 4 and (raw > dmax).any()
    assert got.shape == want.shape and np.array_equal(got, want)
    sim.close()


def test_predefined_profile_runs_through_the_deck(product):
    """profile = predefined / parabolic_channel: a ramp that starts inside the initial window"""
    over = ["electrons.profile=predefined", "electrons.predefined_profile_name=parabolic_channel",
            "electrons.predefined_profile_params=-8*um 6*um 4*um 6*um 10*um n0", "max_step=4"]
    sim = WarpXSim.from_inputs(product, DECK, overrides=over)
    sim.evolve(4)
    got = M.sort_by_position(sim.particles(0))
    p = (-8 * M.UM, 6 * M.UM, 4 * M.UM, 6 * M.UM, 10 * M.UM, 2.e23)
    want, shifts = M.ramp_deck_particles(sim.istep * sim.dt, M.parabolic_channel(p))
    assert shifts >= 1 and want.shape[1] > 1000
    assert got.shape == want.shape and np.array_equal(got[:3], want[:3])
    assert np.max(np.abs(got[3] - want[3])) <= 1e-13 * np.max(want[3])
    sim.close()


def test_parsed_momenta_in_a_boosted_frame_are_no_longer_refused(product):
    """the parent threw `a momentum function evaluated on the host is lab-frame only`: the programs now run on the device"""
    over = ["electrons.momentum_distribution_type=parse_momentum_function",
            "electrons.momentum_function_ux(x,y,z)=0.01*x/8.e-6", "electrons.momentum_function_uy(x,y,z)=0.",
            "electrons.momentum_function_uz(x,y,z)=0.", "max_step=6"]
    sim = WarpXSim.from_inputs(product, os.path.join(DECKS, "boosted_injection_3d.inputs"), overrides=over)
    sim.evolve(6)
    p = sim.particles(0)
    assert p.shape[1] > 0
    live = p[3] > 0
    assert live.any() and np.ptp(p[4][live]) > 0.001 * M.C_LIGHT   # u_x follows x
    sim.close()


def test_other_profiles_are_refused_by_name(product):
    with pytest.raises(_capi.WxaError) as err:
        WarpXSim.from_inputs(product, DECK, overrides=["electrons.profile=from_file"])
    msg = str(err.value)
    assert "profile must be constant" not in msg
    assert "fromfile" in msg and "constant, parse_density_function, predefined" in msg
