"""tests/spline_model.py by itself, and the CPU oracle pinned to it.

The parity tests compare the HIP kernels with the oracle, and the oracle is tied to the reference through deck checksums
that use particle shapes 1 and 3, Galerkin gathering and, for the direct deposition, order 1 only.  Orders 2 and 4, the
plain gather and the direct deposition above order 1 are pinned here instead: to the definitions (cardinal B-splines,
Esirkepov's formula), in extended precision, in a box with an index offset and a 2 mm physical offset as well as in the
suite's usual one."""
from fractions import Fraction

import numpy as np
import pytest

from tests import helpers as H
from tests import spline_model as M
from warpx_amd import plasma

LD = M.LD

# ncell, box_lo, prob_lo, dx: the offset box, and the one every kernel test uses (H.geom_for)
OFFSET_BOX = ((13, 7, 9), (5, -3, 100), (1e-6, -3e-6, 2e-3), (0.5e-6, 0.4e-6, 0.25e-6))
SUITE_BOX = ((24, 20, 16), (0, 0, 0), (-H.LX / 2,) * 3, tuple(H.LX / np.array((24, 20, 16))))
BOXES = {"offset_13x7x9": OFFSET_BOX, "suite_24x20x16": SUITE_BOX}
NPART = 300


def test_extended_precision_is_available():
    """The gates below are in units the oracle's own double rounding sets; the model has to sit well under them."""
    assert np.finfo(LD).eps < 2e-19


@pytest.mark.parametrize("n,at,value", [
    (0, 0, 1), (1, 0, 1), (2, 0, Fraction(3, 4)), (3, 0, Fraction(2, 3)), (4, 0, Fraction(115, 192)),
    (2, Fraction(1, 2), Fraction(1, 2)), (2, 1, Fraction(1, 8)), (3, 1, Fraction(1, 6)), (3, Fraction(1, 2), Fraction(23, 48)),
    (4, 1, Fraction(19, 96)), (4, 2, Fraction(1, 384)), (4, Fraction(1, 2), Fraction(11, 24))])
def test_bspline_values(n, at, value):
    """B_n at the points where it is a textbook fraction (B_n(0) = 1, 3/4, 2/3, 115/192; the integer and half-integer
    samples of the quadratic, cubic and quartic)."""
    t = LD(at.numerator) / LD(at.denominator) if isinstance(at, Fraction) else LD(at)
    want = LD(value.numerator) / LD(value.denominator) if isinstance(value, Fraction) else LD(value)
    for sign in (1, -1):
        if n == 0 and at != 0:
            continue
        assert abs(M.bspline(n, np.array([sign * t]))[0] - want) < 4 * np.finfo(LD).eps


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4])
def test_bspline_partition_of_unity_symmetry_and_support(n):
    rng = np.random.default_rng(n)
    t = (rng.random(2000) - 0.5).astype(LD)
    shifts = np.arange(-4, 5).astype(LD)
    total = M.bspline(n, t[:, None] - shifts[None, :]).sum(axis=1)
    assert np.max(np.abs(total - 1)) < 8 * np.finfo(LD).eps
    s = (6 * rng.random(2000) - 3).astype(LD)
    assert np.max(np.abs(M.bspline(n, s) - M.bspline(n, -s))) < 8 * np.finfo(LD).eps
    assert np.all(M.bspline(n, s) >= 0)
    half = LD(n + 1) / 2
    assert not np.any(M.bspline(n, np.array([half, half + 1, -half - LD(1) / 1000])))
    if n == 0:   # the top-hat is closed on the left: a particle on a cell's lower face belongs to that cell
        assert M.bspline(0, np.array([-LD(1) / 2]))[0] == 1 and M.bspline(0, np.array([LD(1) / 2]))[0] == 0
    # integral 1 (midpoint rule on a grid that resolves every polynomial piece exactly enough)
    x = (np.arange(-4000, 4000) + 0.5).astype(LD) / 1000
    assert abs(M.bspline(n, x).sum() / 1000 - 1) < 1e-6


@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("u_scale", [1.0, 0.003])
def test_model_esirkepov_satisfies_continuity_with_the_model_charge(order, u_scale):
    """(rho_new - rho_old) / dt + div J = 0 with the model's own current and the model's own charge at the old and new
    positions, to extended-precision rounding: the property that makes the model a reference without any library."""
    case = H.geom_case(*OFFSET_BOX)
    parts = case.random_particles(NPART, 50 + order, u_scale)
    _, ng_depos, ng_j = H.guard_depths(order, use_filter=True)
    g = case.geom(ng_depos)
    dt = H.yee_dt(case.dx)
    q = -plasma.Q_E
    J = [case.field(n, ng_j) for n in ("jx", "jy", "jz")]
    rho = case.field("rho", ng_j)
    jx, jy, jz = M.deposit_esirkepov(parts, g, J, q, dt, -0.5 * dt, order)
    old, new = M.esirkepov_positions(parts, dt, -0.5 * dt)
    rho_old, rho_new = M.charge(parts, g, rho, q, order, x=old), M.charge(parts, g, rho, q, order, x=new)
    dx = [1 / LD(g.dinv[d]) for d in range(3)]
    A, B, Cc = jx.shape[0], jy.shape[1], jz.shape[2]
    div = ((jx[1:A] - jx[0:A - 1])[:, 1:B, 1:Cc] / dx[0] + (jy[:, 1:B] - jy[:, 0:B - 1])[1:A, :, 1:Cc] / dx[1]
           + (jz[:, :, 1:Cc] - jz[:, :, 0:Cc - 1])[1:A, 1:B, :] / dx[2])
    drho = (rho_new - rho_old)[1:A, 1:B, 1:Cc] / LD(dt)
    resid = float(np.max(np.abs(drho + div)) / np.max(np.abs(drho)))
    print(f"model continuity order {order} u_scale {u_scale}: {resid:.2e}")
    # a thousand roundings of the extended format, amplified by 1 / u_scale where J is a difference of nearly equal
    # weights; double arithmetic anywhere in the model would leave 1e-15 / u_scale
    assert resid < 1000 * np.finfo(LD).eps / u_scale


CASES = [(op, order, box, lattice) for op in M.OPS for order in (1, 2, 3, 4) for box in BOXES for lattice in (False, True)]


def oracle_error(oracle, op, order, box, lattice):
    case = H.geom_case(*BOXES[box])
    parts = M.case_particles(case, op, NPART, 100 * order + len(op), lattice)
    return M.library_error(oracle, "cpu", op, order, case, parts)


@pytest.mark.parametrize("op,order,box,lattice", CASES)
def test_oracle_against_the_model(oracle, op, order, box, lattice):
    """Charge, the gather of E and of B (read through push_p: with u = 0 and B = 0 the Boris push leaves q dt / m . E; with
    E = 0 the rotation of a known u by B), Galerkin and plain, the direct and the Esirkepov deposition (u ~ c and
    u ~ 0.003 c), orders 1-4, uniform positions and the half-cell lattice, both boxes.  Gate: ten times the worst figure
    measured for the operation and order (spline_model.MEASURED), never above the parity gate of HIP against oracle."""
    err = oracle_error(oracle, op, order, box, lattice)
    print(f"oracle vs model {op} order {order} {box} lattice={lattice}: {err:.2e} (gate {M.gate(op, order):.1e})")
    assert err < M.gate(op, order)
