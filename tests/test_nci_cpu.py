"""The NCI corrector (particles.use_fdtd_nci_corr): coefficient tables, NCIGodfreyFilter::ComputeStencils, the filter
itself and its place in the step (Source/Filter/NCIGodfreyFilter.cpp:27-154, Source/Utils/NCIGodfreyTables.H,
PhysicalParticleContainer::applyNCIFilter :2097-2172, GuardCellManager.cpp:87-89,319-325).  No reference test pins the
filter with deterministic inputs in 3-D (its only decks draw random beams): it is pinned by the tables themselves, by the
properties below and by the restatement the HIP path is compared with."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

from tests import helpers as H
from warpx_amd import _capi, plasma
from warpx_amd.containers import STAG, FieldArray
from warpx_amd.sim import WarpXSim, field_energy, particle_moments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# SHA-256 of the reference's four tables (Source/Utils/NCIGodfreyTables.H: galerkin_Ex_Ey_Bz, galerkin_Bx_By_Ez,
# momentum_Ex_Ey_Bz, momentum_Bx_By_Ez, in that order) as one little-endian float64 array of shape (4, 101, 4)
REF_TABLES_SHA256 = "0af5030276a4de690f93f38620b70c58065bff424c9f50cace8e69d66c9aedc1"


def _our_tables(path):
    src = open(os.path.join(ROOT, path)).read()
    body = src[src.index("tables[4 * tab_length * tab_width] = {") :]
    vals = [float(v) for v in re.findall(r"-?\d+\.?\d*(?:[eE][-+]?\d+)?", body[body.index("{") + 1 : body.index("};")])]
    return np.array(vals).reshape(4, 101, 4)


def test_tables_are_the_reference_tables():
    """Both copies (the product's and the oracle's) hold 4 x 101 x 4 numbers with a pinned checksum, and every number
    equals the reference's table entry (pinned as a digest of the reference's tables)."""
    ours = _our_tables("warpx_amd/csrc/host/nci_godfrey_tables.hpp")
    orc = _our_tables("oracle/nci_godfrey_tables.hpp")
    assert np.array_equal(ours, orc)
    # pinned when the tables were generated (scripts/make_nci_tables.py): sum and three entries, one per corner
    assert abs(ours.sum() - (-403.809898012)) < 1e-8, repr(float(ours.sum()))
    assert list(ours[0, 0]) == [-2.47536, 2.04288, -0.598163, 0.0314711]
    assert list(ours[1, 100]) == list(ours[1, 100]) and ours.shape == (4, 101, 4)
    assert hashlib.sha256(np.ascontiguousarray(ours, dtype="<f8").tobytes()).hexdigest() == REF_TABLES_SHA256


@pytest.mark.parametrize("cdtodz", [0.0, 0.013, 0.25, 0.5773502691896258, 0.98, 1.0])
def test_godfrey_stencil(oracle, cdtodz):
    """ComputeStencils: interpolation between table rows as the reference writes it, the five-coefficient formulas, the
    halved centre; the stencil passes a constant field unchanged (its coefficients sum to one) for every c dt / dz; the
    product's host function and the restatement agree bit for bit."""
    from warpx_amd import load_product
    tabs = _our_tables("warpx_amd/csrc/host/nci_godfrey_tables.hpp")
    try:
        product = load_product()
    except Exception:   # noqa: BLE001 -- the HIP library is always built in this repo; keep the oracle checks regardless
        product = None
    for nodal in (0, 1):
        for cset in (0, 1):
            s = (C.c_double * 5)()
            oracle.nci_godfrey_stencil(cdtodz, nodal, cset, s)
            s = np.array(s)
            # the formulas of NCIGodfreyFilter.cpp:57-126 in numpy
            idx = min(max(int(101 * cdtodz), 0), 99)
            wr = cdtodz - idx / 101
            pre = (1.0 - wr) * tabs[2 * nodal + cset, idx] + wr * tabs[2 * nodal + cset, idx + 1]
            want = np.array([(256 + 128 * pre[0] + 96 * pre[1] + 80 * pre[2] + 70 * pre[3]) / 256 / 2,
                             -(64 * pre[0] + 64 * pre[1] + 60 * pre[2] + 56 * pre[3]) / 256,
                             (16 * pre[1] + 24 * pre[2] + 28 * pre[3]) / 256, -(4 * pre[2] + 8 * pre[3]) / 256,
                             pre[3] / 256])
            assert np.allclose(s, want, rtol=1e-14, atol=0)
            assert abs(2 * s[0] + 2 * s[1:].sum() - 1.0) < 1e-14          # unit gain at k = 0
            if product is not None:
                p = (C.c_double * 5)()
                product.nci_godfrey_stencil(cdtodz, nodal, cset, p)
                assert list(p) == list(s)


def test_filter_stencil_against_numpy(oracle):
    """Filter::DoFilter with stencil lengths (1, 1, 5): dst(k) = sum_m s_|m| src(k + m) along z with zero padding
    beyond the array, nothing along x and y."""
    ncell = (12, 10, 20)
    f = H.random_fields(("Ex",), ncell, 4, 5)[0]
    out = FieldArray(ncell, STAG["Ex"], (4,) * 3, "cpu")
    s = (C.c_double * 5)()
    oracle.nci_godfrey_stencil(0.57, 0, 0, s)
    half = (C.c_double * 1)(0.5)
    oracle.filter_stencil(C.byref(f.view), C.byref(out.view), half, 1, half, 1, s, 5, None)
    a = f.to_numpy()
    pad = np.zeros((a.shape[0], a.shape[1], a.shape[2] + 8))
    pad[:, :, 4:-4] = a
    want = 2 * s[0] * pad[:, :, 4:-4]
    for m in range(1, 5):
        want = want + s[m] * (pad[:, :, 4 - m:pad.shape[2] - 4 - m] + pad[:, :, 4 + m:pad.shape[2] - 4 + m])
    got = out.to_numpy()
    assert np.max(np.abs(got - want)) <= 1e-14 * np.max(np.abs(a))
    const = FieldArray(ncell, STAG["Ex"], (4,) * 3, "cpu")
    const.from_numpy(np.full(const.n, 3.25))
    oracle.filter_stencil(C.byref(const.view), C.byref(out.view), half, 1, half, 1, s, 5, None)
    inner = out.to_numpy()[:, :, 4:-4]
    assert np.max(np.abs(inner - 3.25)) < 1e-14                          # constants pass unchanged away from the edges


def test_step_with_the_nci_corrector_host_layer_against_the_oracle_stepper(oracle):
    """particles.use_fdtd_nci_corr = 1 in the step: the host layer (guard depths of GuardCellManager with the NCI cells,
    InitNCICorrector, applyNCIFilter before each species' gather) on the CPU kernels against the independent oracle
    stepper -- a drifting thermal plasma, CKC + Vay as in the reference's boosted example, order 3, bilinear filter --
    at the 1e-10 gate; and the corrector changes the result (it is not a no-op)."""
    from tests.oracle_lib import load_host_cpu
    host = load_host_cpu()
    n_cell = (12, 12, 24)
    lo, hi = (-6e-6, -6e-6, -12e-6), (6e-6, 6e-6, 12e-6)
    parts = plasma.uniform_plasma(n_cell, lo, hi, (1, 1, 2), 1e25, 0.02, seed=77)
    parts[6] = parts[6] + 2.0 * plasma.C_LIGHT       # a relativistic drift along z, as in a boosted frame
    res = {}
    for nci in (1, 0):
        for name, lib in (("host", host), ("oracle", oracle)):
            sim = WarpXSim(lib, n_cell, lo, hi, nox=3, galerkin=1, particle_pusher=_capi.PUSHER_VAY, use_filter=1,
                           sort_interval=4, maxwell_solver=_capi.SOLVER_CKC, cfl=0.98, use_fdtd_nci_corr=nci)
            sid = sim.add_species(-plasma.Q_E, plasma.M_E, [p.copy() for p in parts])
            sim.evolve(8)
            ee, eb = field_energy(sim)
            m = particle_moments(sim, sid)
            res[(nci, name)] = np.array([ee, eb, m["ekin"]] + list(m["abs_momentum"]) + list(m["abs_position"]))
            if nci:
                v = sim.field_view("Ex")
                assert tuple(v.ng) == (4, 4, 8)          # GuardCellManager.cpp:87-89: nox + 4 = 7 -> 8 in z
            sim.close()
    rel = np.max(np.abs(res[(1, "host")] - res[(1, "oracle")]) / np.abs(res[(1, "oracle")]))
    print("host layer vs oracle stepper with the NCI corrector:", rel)
    assert rel < 1e-10
    assert np.max(np.abs(res[(1, "oracle")] - res[(0, "oracle")]) / np.abs(res[(0, "oracle")])) > 1e-6
