"""Density profiles without a GPU: tests/decks/density_ramp_window_3d.inputs through the host layer on the CPU backend,
which has no add_plasma_profile entry and takes the host loop of PhysicalParticleContainer::AddPlasma (Parser::eval,
the 27-point probe, density_min / density_max); wxa_expr_compile and the host evaluation of the compiled program; the
deck reader's refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import plasma_profile_model as M
from tests.oracle_lib import load_host_cpu
from tests.test_expr_device_gpu import CLOSE, CONSTANTS, EXACT
from warpx_amd import _capi
from warpx_amd.sim import WarpXSim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECKS = os.path.join(ROOT, "tests", "decks")
DECK = os.path.join(DECKS, "density_ramp_window_3d.inputs")


@pytest.fixture(scope="module")
def lib():
    return load_host_cpu()


@pytest.fixture(scope="module")
def product():
    if not os.path.exists(_capi.PRODUCT_LIB):
        import __graft_entry__ as g
        g.build()
    return _capi.load_product()


def test_ramp_deck_on_the_host_loop_gives_the_models_particles(lib):
    sim = WarpXSim.from_inputs(lib, DECK)
    sim.evolve(sim.max_step)
    got = M.sort_by_position(sim.particles(0))
    want, shifts = M.ramp_deck_particles(sim.istep * sim.dt)
    assert shifts > 32 and want.shape[1] > 10000
    assert got.shape == want.shape
    assert np.array_equal(got[:4], want[:4]) and np.all(got[4:] == 0.0)
    sim.close()


def test_density_min_and_max_on_the_host_loop(lib):
    """the foot is dropped, the top is clipped: thresholds between the densities of two lattice planes (the model
    asserts the margin)"""
    n0 = 2.e23
    over = ["electrons.density_min=0.2*n0", "electrons.density_max=0.9*n0", "max_step=48"]
    sim = WarpXSim.from_inputs(lib, DECK, overrides=over)
    sim.evolve(48)
    got = M.sort_by_position(sim.particles(0))
    free, _ = M.ramp_deck_particles(sim.istep * sim.dt)
    dv = M.UM * M.UM * (M.UM / 2)
    dens = M.ramp_deck_density(free[0], free[1], free[2])
    for thr in (0.2 * n0, 0.9 * n0):
        assert np.min(np.abs(dens - thr)) > 1e-9 * thr
    keep = dens >= 0.2 * n0
    assert 0 < keep.sum() < dens.size and (dens > 0.9 * n0).any()
    want_w = np.where(0.9 * n0 < dens[keep], 0.9 * n0, dens[keep]) * (dv / 2)
    assert got.shape[1] == int(keep.sum())
    assert np.array_equal(got[:3], free[:3, keep]) and np.array_equal(got[3], want_w)
    sim.close()


def test_predefined_profile_on_the_host_loop(lib):
    over = ["electrons.profile=predefined", "electrons.predefined_profile_name=parabolic_channel",
            "electrons.predefined_profile_params=-8*um 6*um 4*um 6*um 10*um n0", "max_step=4"]
    sim = WarpXSim.from_inputs(lib, DECK, overrides=over)
    sim.evolve(4)
    got = M.sort_by_position(sim.particles(0))
    p = (-8 * M.UM, 6 * M.UM, 4 * M.UM, 6 * M.UM, 10 * M.UM, 2.e23)
    want, _ = M.ramp_deck_particles(sim.istep * sim.dt, M.parabolic_channel(p))
    assert want.shape[1] > 1000 and got.shape == want.shape and np.array_equal(got[:3], want[:3])
    assert np.max(np.abs(got[3] - want[3])) <= 1e-13 * np.max(want[3])   # libm's cos against numpy's
    sim.close()


@pytest.mark.parametrize("over,words", [
    (["electrons.profile=from_file"], ["fromfile", "constant, parse_density_function, predefined"]),
    (["electrons.profile=predefined", "electrons.predefined_profile_name=gaussian_blob",
      "electrons.predefined_profile_params=1 2 3 4 5 6"], ["gaussian_blob", "parabolic_channel"]),
    (["electrons.profile=predefined", "electrons.predefined_profile_name=parabolic_channel",
      "electrons.predefined_profile_params=1 2 3 4 5"], ["takes 6 values", "got 5"]),
    (["electrons.profile=predefined"], ["predefined_profile_name must be set"]),
    (["electrons.density_function(x,y,z)=n0*nope"], ["unknown name 'nope'"]),
    (["electrons.momentum_distribution_type=gaussian_parse_momentum_function"], ["gaussianparsemomentumfunction", "not on this path"]),
])
def test_deck_refusals(lib, over, words):
    with pytest.raises(_capi.WxaError) as err:
        WarpXSim.from_inputs(lib, DECK, overrides=over)
    for w in words:
        assert w in str(err.value), str(err.value)
    assert "profile must be constant" not in str(err.value)


def test_the_host_loop_stays_lab_frame_only(lib):
    over = ["electrons.profile=parse_density_function", "electrons.density_function(x,y,z)=1.e6*(z>=1.e-6)"]
    with pytest.raises(_capi.WxaError, match="lab-frame only"):
        WarpXSim.from_inputs(lib, os.path.join(DECKS, "boosted_injection_3d.inputs"), overrides=over)


KNOWN = {"-2^2": -4.0, "2**-1": 0.5, "heaviside(0,0.5)": 0.5, "fmod(-7.5,2)": -1.5, "2^3^2": 512.0, "3.5": 3.5}


@pytest.mark.parametrize("text", EXACT + CLOSE)
def test_compiled_expressions_evaluate_like_the_decks_parser(product, text):
    """wxa_expr_compile + wxa_expr_eval_host against wxa_parser_eval, which parses the text anew at every call"""
    e = _capi.Expr(product, text, ("x", "y"), CONSTANTS)
    nops, depth = e.info()
    assert 1 <= nops <= 256 and 1 <= depth <= 16
    names = (C.c_char_p * 4)(b"x", b"y", *[k.encode() for k in CONSTANTS])
    for x, y in ((0.0, 1.0), (2.5, 0.5), (-3.0, 4.0), (1.0, 1.0)):
        vals = (C.c_double * 4)(x, y, *CONSTANTS.values())
        out = C.c_double()
        product.parser_eval(text.encode(), 4, names, vals, C.byref(out))
        got = e.eval_host(x, y)
        assert got == out.value or (np.isnan(got) and np.isnan(out.value)), (text, x, y, got, out.value)
        if text in KNOWN:
            assert got == KNOWN[text]
    e.close()
