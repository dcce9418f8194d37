"""PhysicalParticleContainer::AddPlasma with a density profile, restated in numpy for the tests of
wxa_add_plasma_profile and of the decks that reach it (Source/Particles/PhysicalParticleContainer.cpp:1015-1051 the cell
probe, :1175-1276 the particle loop, :138-148 applyBallisticCorrection; Source/Initialization/InjectorPosition.H:74-92
the regular lattice; InjectorDensity.H:82-107 parabolic_channel).

Every numpy ufunc rounds once, like the statement it restates: the lattice is corner + (i + r) * dx, the weight
density * (dx dy dz / nppc).  Densities and momenta are numpy functions of (x, y, z) written by the test, never the
project's parser."""
import math

import numpy as np

C_LIGHT = 299792458.0
Q_E, M_E, EP0 = 1.602176634e-19, 9.1093837015e-31, 8.8541878128e-12
FLT_MAX = np.finfo(np.float64).max


def parabolic_channel(p):
    """InjectorDensityPredefined::getDensity, parabolic_channel, in the reference's operation order"""
    z_start, ramp_up, plateau, ramp_down, rc, n0 = (float(v) for v in p)
    kp = Q_E / C_LIGHT * math.sqrt(n0 / (M_E * EP0))

    def density(x, y, z):
        zs = z - z_start
        up = 0.5 * (1. - np.cos(np.pi * zs / ramp_up))
        down = 0.5 * (1. + np.cos(np.pi * (zs - ramp_up - plateau) / ramp_down))
        n = np.where((zs >= 0) & (zs < ramp_up), up,
                     np.where((zs >= ramp_up) & (zs < ramp_up + plateau), 1.,
                              np.where((zs >= ramp_up + plateau) & (zs < ramp_up + plateau + ramp_down), down, 0.)))
        return n * (n0 * (1. + 4. * (x * x + y * y) / (kp * kp * rc * rc * rc * rc)))
    return density


def add_plasma(density, *, corner, ncells, dx, ppc, lo, hi, brick_lo, brick_hi, momentum=None, gamma_boost=1.0, t=0.0,
               density_min=0.0, density_max=FLT_MAX):
    """The particles (7, n) -- x y z w ux uy uz -- of the cells [0, ncells) above `corner`, sorted by position, and the
    density at each of them before threshold and cap."""
    beta = math.sqrt(1.0 - 1.0 / math.pow(gamma_boost, 2.0)) if gamma_boost > 1.0 else 0.0
    ct = C_LIGHT * t

    def bulk(x, y, z):
        if momentum is None:
            return np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
        return tuple(np.broadcast_to(f(x, y, z), x.shape).astype(np.float64) for f in momentum)

    def ballistic(x, y, z):   # applyBallisticCorrection with the bulk momentum at (x, y, z)
        ux, uy, uz = bulk(x, y, z)
        gamma_bulk = np.sqrt(1.0 + (ux * ux + uy * uy + uz * uz))
        betaz = uz / gamma_bulk
        return gamma_boost * (z * (1.0 - beta * betaz) - ct * (betaz - beta))

    def inside(x, y, z):      # InjectorPosition::insideBounds
        return (x < hi[0]) & (x >= lo[0]) & (y < hi[1]) & (y >= lo[1]) & (z < hi[2]) & (z >= lo[2])

    i, j, k = np.meshgrid(np.arange(ncells[0]), np.arange(ncells[1]), np.arange(ncells[2]), indexing="ij")
    iv = [i.ravel(), j.ravel(), k.ravel()]
    clo = [corner[d] + (iv[d] + 0.0) * dx[d] for d in range(3)]
    chi = [corner[d] + (iv[d] + 1.0) * dx[d] for d in range(3)]
    clo[2], chi[2] = ballistic(*clo), ballistic(*chi)
    emits = np.ones(iv[0].shape, dtype=bool)
    for d in range(3):        # overlapsWith
        emits &= ~((clo[d] > hi[d]) | (chi[d] < lo[d]))
    lim = [(clo[d], (clo[d] + chi[d]) / 2., chi[d]) for d in range(3)]
    found = np.zeros_like(emits)
    for px in lim[0]:
        for py in lim[1]:
            for pz in lim[2]:
                with np.errstate(all="ignore"):
                    found |= inside(px, py, pz) & (density(px, py, pz) > 0)
    emits &= found

    nppc = ppc[0] * ppc[1] * ppc[2]
    scale_fac = dx[0] * dx[1] * dx[2] / nppc
    rows = []
    for ip in range(nppc):    # getPositionUnitBox
        ix = ip // (ppc[1] * ppc[2])
        iz = (ip - ix * ppc[1] * ppc[2]) // ppc[1]
        iy = (ip - ix * ppc[1] * ppc[2]) - ppc[1] * iz
        r = ((0.5 + ix) / ppc[0], (0.5 + iy) / ppc[1], (0.5 + iz) / ppc[2])
        pos = [corner[d] + (iv[d] + r[d]) * dx[d] for d in range(3)]
        ok = emits.copy()
        for d in range(3):    # tile_realbox.contains: strictly inside
            ok &= (pos[d] > brick_lo[d]) & (pos[d] < brick_hi[d])
        x, y, z = (p[ok] for p in pos)
        z0 = ballistic(x, y, z)
        ok = inside(x, y, z0)
        x, y, z, z0 = x[ok], y[ok], z[ok], z0[ok]
        with np.errstate(all="ignore"):
            dens = np.broadcast_to(density(x, y, z0), x.shape).astype(np.float64)
        raw = dens
        ok = ~(dens < density_min)
        x, y, z, z0, dens, raw = x[ok], y[ok], z[ok], z0[ok], dens[ok], raw[ok]
        dens = np.where(density_max < dens, density_max, dens)
        if gamma_boost > 1.0:
            ux, uy, uz = bulk(x, y, np.zeros_like(x))
            gamma_lab = np.sqrt(1.0 + (ux * ux + uy * uy + uz * uz))
            betaz_lab = uz / gamma_lab
            dens = gamma_boost * dens * (1.0 - beta * betaz_lab)
            uz = gamma_boost * (uz - beta * gamma_lab)
        else:
            ux, uy, uz = bulk(x, y, z0)
        rows.append(np.stack([x, y, z, dens * scale_fac, ux * C_LIGHT, uy * C_LIGHT, uz * C_LIGHT, raw]))
    out = np.concatenate(rows, axis=1)
    out = out[:, np.lexsort(out[:3])]
    return out[:7], out[7]


def sort_by_position(p):
    return p[:, np.lexsort(p[:3])]


# ---- tests/decks/density_ramp_window_3d.inputs ----
UM = 9.5367431640625e-07   # 2^-20 m: the deck's unit of length


def ramp_deck_density(x, y, z):
    n0, zs, length, rc = 2.e23, 2 * UM, 24 * UM, 10 * UM
    return n0 * (z - zs) / length * (1 + 4 * (x * x + y * y) / (rc * rc)) * (z >= zs)


def ramp_deck_particles(t, density=ramp_deck_density):
    """What the deck's window holds at time t: the window has moved by whole cells, floor(c t / dz) of them (the test
    checks that c t / dz is not within rounding of a whole number); the plasma at rest that entered is the injection
    lattice of the window's cells, the particles behind the window's lower edge are gone.  Returns (particles, shifts)."""
    dx = (UM, UM, UM / 2)
    shifts = int(math.floor(C_LIGHT * t / dx[2]))
    frac = C_LIGHT * t / dx[2] - shifts
    assert 1e-6 < frac < 1 - 1e-6
    corner = (-8 * UM, -8 * UM, (-32 + shifts) * dx[2])
    top = (8 * UM, 8 * UM, shifts * dx[2])
    p, _ = add_plasma(density, corner=corner, ncells=(16, 16, 32), dx=dx, ppc=(1, 1, 2), lo=(-FLT_MAX,) * 3,
                      hi=(FLT_MAX,) * 3, brick_lo=corner, brick_hi=top)
    return p, shifts
