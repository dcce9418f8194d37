"""tests/pusher_model.py by itself, and the CPU oracle pinned to it per particle.

The parity tests of the momentum push compare the HIP kernels with the oracle in one regime (|u| ~ c, a rotation angle of
1e-5) under a max-norm over the launch, and the oracle restates the same lines as the kernels.  Here the model is first
held against facts that none of the restated formulas supplies (conservation, the rotation angle, the force-free orbit, the
radiated power), then the oracle against the model over cold, thermal and beam momenta, field-free to strongly
magnetised, three species, with an error per particle in units of 2^-53 of that particle's own momentum and kick."""
import numpy as np
import pytest

from tests import pusher_model as M
from warpx_amd import plasma

LD = M.LD
EPS = np.finfo(LD).eps
C = plasma.C_LIGHT
DT = M.box_dt()
N = 500


def _gaussian_u(scale, seed, n=N):
    return scale * C * np.random.default_rng(seed).standard_normal((3, n))


def _rel(a, b, scale):
    return float(np.max(M.norm(a - b) / scale))


def test_extended_precision_is_available():
    assert EPS < 2e-19


def test_classical_electron_radius():
    """The one constant read from the C++ sources is q_e^2 / (4 pi eps0 m_e c^2) to the digits of eps0."""
    assert abs(M.R_E / (plasma.Q_E ** 2 / (4 * np.pi * plasma.EP0 * plasma.M_E * C ** 2)) - 1) < 1e-9


@pytest.mark.parametrize("species", list(M.SPECIES))
@pytest.mark.parametrize("u_over_c", M.U_OVER_C)
def test_without_b_the_kick_is_q_e_dt_over_m(species, u_over_c):
    """B = 0: Boris, Vay and Higuera-Cary add q E dt / m.  The radiation-reaction pusher adds the Landau-Lifshitz force at
    the midpoint on top, which for B = 0 is -K gamma^2 beta E_perp^2 along the velocity and K beta E_par E_perp across it
    (K = 2/3 r_e (q / m c)^2): the three terms of the force written out in the velocity's own frame."""
    q, m = M.SPECIES[species]
    E = np.array((3e11, -1e12, 5e11))
    u = M.vec(_gaussian_u(u_over_c, 1))
    kick = LD(q) * LD(DT) / LD(m) * M.vec(E)
    scale = M.norm(u) + M.norm(kick)
    for name in ("boris", "vay", "hc"):
        assert _rel(M.push(name, u, E, np.zeros(3), q, m, DT), u + kick, scale) < 8 * EPS, name
    mid = u + kick / 2
    gamma = M.lorentz_factor(mid)
    beta = M.norm(mid) / gamma / LD(C)
    bhat = mid / M.norm(mid)
    e_par = M.dot(M.vec(E), bhat)
    e_perp = M.vec(E) - e_par * bhat
    K = 2 * LD(M.R_E) / 3 * (LD(q) / (LD(m) * LD(C))) ** 2
    want = K * (-gamma ** 2 * beta * M.dot(e_perp, e_perp) * bhat + beta * e_par * e_perp)
    got = (M.push("rr", u, E, np.zeros(3), q, m, DT) - (u + kick)) / LD(DT)
    # against the largest term of the bracket, gamma^2 beta E^2 (the terms along the velocity cancel down to E_perp^2);
    # `got` is a difference of momenta, so the radiated momentum must not drown in the rounding of u + kick
    force_scale = K * gamma ** 2 * beta * M.dot(M.vec(E), M.vec(E))
    resolved = scale * EPS / LD(DT)
    assert float(np.max(M.norm(got - want) / (64 * EPS * force_scale + 8 * resolved))) < 1.0


@pytest.mark.parametrize("tau", [1e-5, 1e-2, 1.0, 4.0, 4e3])
@pytest.mark.parametrize("u_over_c", M.U_OVER_C)
def test_without_e_the_magnitude_is_kept_and_boris_turns_by_its_angle(tau, u_over_c):
    """E = 0: the three Lorentz pushers keep |u|; Boris turns the part of u across B by 2 atan(|q| B dt / (2 m gamma))
    about B, clockwise for a positive charge."""
    for species in ("electron", "proton"):
        q, m = M.SPECIES[species]
        B = M.D_B_OBLIQUE * M._b_for_half_angle(tau, q, m)
        u = M.vec(_gaussian_u(u_over_c, 2))
        for name in ("boris", "vay", "hc"):
            out = M.push(name, u, np.zeros(3), B, q, m, DT)
            # Boris turns by construction; in the other two a rounding of the part along B enters a cross product with
            # t = tau / gamma, so their |u| holds to a rounding times the rotation's parameter
            tol = 16 * EPS * (1 if name == "boris" else 1 + tau)
            assert float(np.max(np.abs(M.norm(out) / M.norm(u) - 1))) < tol, (name, species)
        out = M.push("boris", u, np.zeros(3), B, q, m, DT)
        bhat = M.vec(B) / M.norm(M.vec(B))
        perp_in, perp_out = u - M.dot(u, bhat) * bhat, out - M.dot(out, bhat) * bhat
        assert _rel(M.dot(out, bhat), M.dot(u, bhat), M.norm(u)) < 16 * EPS      # the part along B stays
        theta = 2 * np.arctan(abs(LD(q)) * M.norm(M.vec(B)) * LD(DT) / (2 * LD(m) * M.lorentz_factor(u)))
        p2 = M.dot(perp_in, perp_in)
        assert float(np.max(np.abs(M.dot(perp_in, perp_out) / p2 - np.cos(theta)))) < 32 * EPS
        sense = M.dot(M.cross(perp_in, perp_out), bhat) / p2
        assert float(np.max(np.abs(sense + np.sign(q) * np.sin(theta)))) < 32 * EPS


@pytest.mark.parametrize("species", list(M.SPECIES))
@pytest.mark.parametrize("tau", [1e-3, 1.0, 4.0])
def test_force_free_orbit(species, tau):
    """E = -v x B: Vay and Higuera-Cary leave u as it is (the property Vay's pusher was built for); Boris does not."""
    q, m = M.SPECIES[species]
    B = M.vec(M.D_B_OBLIQUE * M._b_for_half_angle(tau, q, m))
    u = M.vec(_gaussian_u(3.0, 3))
    E = -M.cross(u / M.lorentz_factor(u), B)           # per particle, in extended precision
    kick = abs(LD(q)) * LD(DT) / LD(m) * M.norm(E)
    for name in ("vay", "hc"):
        out = M.PUSHERS[name][0](u, E, B, q, m, DT)
        assert float(np.max(M.norm(out - u) / (M.norm(u) + kick))) < 16 * EPS, name
    out = M.PUSHERS["boris"][0](u, E, B, q, m, DT)
    assert float(np.median(M.norm(out - u) / M.norm(u))) > 1e-3 * min(tau, 1.0) ** 3


@pytest.mark.parametrize("pusher", list(M.PUSHERS))
def test_degenerate_inputs(pusher):
    """u along B without E: unchanged.  u = 0 without fields: exactly 0."""
    for species in M.SPECIES:
        q, m = M.SPECIES[species]
        for tau in (1e-5, 4.0, 4e3):
            B = M.D_B_OBLIQUE * M._b_for_half_angle(tau, q, m)
            u = M.vec(B)[:, :1] / M.norm(M.vec(B)) * (LD(C) * np.array([1e-8, 1.0, 1e4], dtype=LD))[None, :]
            out = M.push(pusher, u, np.zeros(3), B, q, m, DT)
            # u is along B to a rounding of the extended format, and the rotation turns that rounding by its parameter
            assert float(np.max(M.norm(out - u) / M.norm(u))) < 16 * EPS * (1 + tau), (species, tau)
        out = M.push(pusher, np.zeros((3, 4)), np.zeros(3), np.zeros(3), q, m, DT)
        assert not np.any(out) and out.shape == (3, 4)


def test_radiated_power_in_a_magnetic_field():
    """An electron of gamma = 1e4 across B without E, one small step: gamma m c^2 falls by
    (2/3) r_e gamma^2 v^2 (e B)^2 / (m c) per unit time.  The scheme takes the force at the mean of the old momentum and the
    rotated one, whose magnitude is |u| cos(theta / 2), so the loss differs from the formula at the initial state by the
    square of the rotation angle theta ~ dt (7e-9 here; the term linear in dt, the energy lost within the step, carries
    1 / gamma^2 and is 1e-13).  The difference must shrink at least in proportion to dt, which a wrong coefficient would
    not, and by the analysis above it falls to a quarter when the step is halved."""
    q, m = M.SPECIES["electron"]
    B = np.array((0.0, 0.0, 1e3))
    u = M.vec(np.array((6e3 * C, 8e3 * C, 0.0)))
    gamma = M.lorentz_factor(u)
    v2 = M.dot(u, u) / gamma ** 2
    power = 2 * LD(M.R_E) / 3 * gamma ** 2 * v2 * (LD(q) * LD(1e3)) ** 2 / (LD(m) * LD(C))
    resid = []
    for dt in (DT, DT / 2, DT / 4):
        out = M.push("rr", u, np.zeros(3), B, q, m, dt)
        loss = (gamma - M.lorentz_factor(out)) * LD(m) * LD(C) ** 2 / LD(dt)
        resid.append(float(abs(loss / power - 1)[0, 0]))
    print("radiated power residuals at dt, dt/2, dt/4:", resid)
    assert resid[0] < 1e-3
    for a, b in zip(resid, resid[1:]):
        assert a / b > 1.9              # at least in proportion to dt
        assert 3.8 < a / b < 4.2        # the order of the scheme


def test_position_update_is_the_new_velocity_times_dt():
    u = M.vec(_gaussian_u(1.0, 5))
    d = M.displacement(u, DT)
    speed = M.norm(d) / LD(DT)
    assert np.all(speed < LD(C))
    assert _rel(d * M.lorentz_factor(u), u * LD(DT), M.norm(u) * LD(DT)) < 8 * EPS


def test_the_gate_table_obeys_its_condition():
    """Every gated cell has an entry, a power of two between 16 and 1024; the strong-B cells of Vay and Higuera-Cary are
    the reported ones."""
    for pusher in M.PUSHERS:
        for fields in M.ALL_FIELD_SETS:
            if (pusher, fields) in M.REPORTED:
                continue
            gates = M.GATES[pusher][fields]
            assert len(gates) == len(M.U_OVER_C)
            for g in gates:
                assert 16 <= g <= M.MAX_GATE and g & (g - 1) == 0, (pusher, fields, g)
    assert set(M.REPORTED) >= {("vay", M.STRONG_B), ("hc", M.STRONG_B)}
    assert M.gate_from(3.9) == 16 and M.gate_from(4.1) == 32 and M.gate_from(100) == 512


# ---- the oracle against the model ------------------------------------------------------------------------------------

def oracle_cell(oracle, pusher, fields, species, u_over_c, move=0):
    parts, E, B, q, m, dt, _ = M.launch_inputs(fields, species, u_over_c)
    got = M.oracle_push(oracle, pusher, parts, E, B, q, m, dt, move)
    reported = (pusher, fields) in M.REPORTED
    err, excess = M.judge(got, pusher, fields, species, u_over_c, move, M.MAX_GATE if reported else M.gate(pusher, fields, u_over_c))
    return got, err, excess


@pytest.mark.parametrize("pusher", list(M.PUSHERS))
@pytest.mark.parametrize("fields", M.ALL_FIELD_SETS)
def test_oracle_against_the_model(oracle, pusher, fields):
    """PushP of the oracle on 4096 particles per launch, every species and every u/c of the cell's row.  The table's
    entry is at least four times what the oracle shows here, so the oracle itself has to stay under a quarter of it."""
    reported = (pusher, fields) in M.REPORTED
    for species in M.SPECIES:
        for u_over_c in M.U_OVER_C:
            got, err, _ = oracle_cell(oracle, pusher, fields, species, u_over_c)
            assert np.all(np.isfinite(got[4:7])), (species, u_over_c)
            print(f"oracle vs model {pusher} {fields} {species} u/c={u_over_c:g}: {err.max():.1f} ulp"
                  + (" (reported)" if reported else f" (gate {M.gate(pusher, fields, u_over_c)})"))
            if not reported:
                assert 4 * err.max() <= M.gate(pusher, fields, u_over_c), M.describe(got, pusher, fields, species, u_over_c, err)
            if fields == "none":
                assert not np.any(got[4:7, 0])      # u = 0 without fields stays exactly 0
    if fields == "none" and pusher in ("boris", "vay"):
        # the entry point without external fields is the same push
        import ctypes as Ct
        from warpx_amd.containers import ParticleArrays, field_triplet
        parts, E, B, q, m, dt, _ = M.launch_inputs(fields, "electron", 1.0)
        Ef, Bf, g = M.zero_fields(1)
        pc = ParticleArrays.from_numpy(parts, "cpu")
        oracle.push_p(Ct.byref(pc.view), field_triplet(Ef), field_triplet(Bf), Ct.byref(g), q, m, dt, 1, 1, M.PUSHERS[pusher][1], None)
        assert np.array_equal(pc.to_numpy(), M.oracle_push(oracle, pusher, parts, E, B, q, m, dt, 0))


@pytest.mark.parametrize("pusher", list(M.PUSHERS))
@pytest.mark.parametrize("fields", M.MOVE_FIELD_SETS)
def test_oracle_position_update_against_the_model(oracle, pusher, fields):
    """PushPX: the momenta as above, the positions within one ulp of the box's largest coordinate plus the cell's gate
    on the displacement."""
    for u_over_c in M.MOVE_U_OVER_C:
        got, err, excess = oracle_cell(oracle, pusher, fields, "electron", u_over_c, move=1)
        print(f"oracle vs model, move, {pusher} {fields} u/c={u_over_c:g}: {err.max():.1f} ulp, position {excess.max():.3f} of its bound")
        assert 4 * err.max() <= M.gate(pusher, fields, u_over_c), M.describe(got, pusher, fields, "electron", u_over_c, err)
        assert excess.max() <= 1.0, (u_over_c, int(np.argmax(excess)), excess.max())
