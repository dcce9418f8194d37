// Plasma injection for gfx950: PhysicalParticleContainer::AddPlasma (PhysicalParticleContainer.cpp:924-1333) with the
// injector's constant density (wxa_add_plasma) or a density and, optionally, momenta given as expressions
// (wxa_add_plasma_profile), and the wxa_expr_* entries (host/Parser.hpp programs; expr_device.hpp runs them on the device).
#include "expr_device.hpp"
#include "gather_body.hpp"
#include "workspace.hpp"

#include <map>
#include <string>

namespace wxa {

struct InjectGeom {
    double corner[3], dx[3], blo[3], bhi[3], lo[3], hi[3], u[3], uth[3], origin[3];
    int nc[3], ppc[3];
    double density, scale_fac;
    unsigned long long seed;
    int thermal;
    // boosted frame / ballistic correction: z0 = gamma_boost (z za - zb) (applyBallisticCorrection, :138-148),
    // za = 1 - beta_boost betaz_bulk, zb = c t (betaz_bulk - beta_boost)
    double gamma_boost, beta_boost, za, zb;
};

// Philox4x32-10 (Salmon et al., SC'11): counter-based, so a particle's draws depend on its position only
__device__ __forceinline__ void philox4x32_10(unsigned c[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (unsigned)p1; c[3] = (unsigned)p0; c[0] = n0; c[2] = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
__device__ __forceinline__ double uniform53(unsigned hi, unsigned lo) {   // (0, 1)
    return ((double)((((unsigned long long)hi << 32) | lo) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}
// three standard normal draws for the injection point with the global lattice coordinates (sx, sy, sz)
__device__ __forceinline__ void normal3(unsigned long long seed, int sx, int sy, int sz, double n[3]) {
    unsigned a[4] = {(unsigned)sx, (unsigned)sy, (unsigned)sz, 0u}, b[4] = {(unsigned)sx, (unsigned)sy, (unsigned)sz, 1u};
    philox4x32_10(a, (unsigned)seed, (unsigned)(seed >> 32));
    philox4x32_10(b, (unsigned)seed, (unsigned)(seed >> 32));
    const double r0 = sqrt(-2.0 * log(uniform53(a[0], a[1]))), t0 = 2.0 * M_PI * uniform53(a[2], a[3]);
    const double r1 = sqrt(-2.0 * log(uniform53(b[0], b[1]))), t1 = 2.0 * M_PI * uniform53(b[2], b[3]);
    n[0] = r0 * cos(t0); n[1] = r0 * sin(t0); n[2] = r1 * cos(t1);
}

// ---- what the two particle passes share --------------------------------------------------------------------
// Lattice point t of the cell box: its cell, the cell's indices, its place in the unit cell.  Here and where the callers
// form corner + (iv + r) * dx: the reference's roundings, one per operation (a fused multiply-add differs in the last bit,
// which moves particles off the reference's lattice and can flip a bounds test at a box edge); the pragma follows no call
__device__ __forceinline__ void lattice_point(const InjectGeom& ig, long t, long& cell, int iv[3], double r[3]) {
#pragma clang fp contract(off)
    const int nppc = ig.ppc[0] * ig.ppc[1] * ig.ppc[2];
    cell = t / nppc;
    const int ip = (int)(t % nppc);
    iv[0] = (int)(cell % ig.nc[0]); iv[1] = (int)((cell / ig.nc[0]) % ig.nc[1]); iv[2] = (int)(cell / ((long)ig.nc[0] * ig.nc[1]));
    // InjectorPositionRegular::getPositionUnitBox (Source/Initialization/InjectorPosition.H:74-92)
    const int ny = ig.ppc[1], nz = ig.ppc[2];
    const int ix_part = ip / (ny * nz);
    const int iz_part = (ip - ix_part * (ny * nz)) / ny;
    const int iy_part = (ip - ix_part * (ny * nz)) - ny * iz_part;
    r[0] = (0.5 + ix_part) / ig.ppc[0]; r[1] = (0.5 + iy_part) / ig.ppc[1]; r[2] = (0.5 + iz_part) / ig.ppc[2];
}

// Accepted points take consecutive slots, one atomic per wave.  Every lane of the wave calls it (the ballot); -1 for a
// lane that stores nothing: not accepted, or past the room -- the host sees count > room and reports it.
__device__ __forceinline__ long inject_slot(bool ok, long room, unsigned long long* __restrict__ count) {
    const unsigned long long mask = __ballot(ok);
    if (mask == 0) return -1;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)mask) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(count, (unsigned long long)__popcll(mask));
    base = __shfl(base, leader);
    if (!ok) return -1;
    const long slot = (long)(base + __popcll(mask & ((1ULL << lane) - 1ULL)));
    return slot < room ? slot : -1;
}

// The particle at pos with the lab-frame bulk momentum u (in units of c) and density dens: the thermal draw, the boost,
// the weight.  No contraction pragma: these products and sums are fused where the compiler fuses them.
__device__ __forceinline__ void inject_store(const PV& dst, const InjectGeom& ig, long slot, const double pos[3], double u[3],
                                             double dens) {
    dst.x[slot] = pos[0]; dst.y[slot] = pos[1]; dst.z[slot] = pos[2];
    if (ig.thermal) {
        double n[3];
        // lattice coordinate = cell * ppc + sub-point: (pos - origin) / dx * ppc = integer + 1/2, robust to round-off
        normal3(ig.seed, (int)floor((pos[0] - ig.origin[0]) / ig.dx[0] * ig.ppc[0]),
                (int)floor((pos[1] - ig.origin[1]) / ig.dx[1] * ig.ppc[1]),
                (int)floor((pos[2] - ig.origin[2]) / ig.dx[2] * ig.ppc[2]), n);
        u[0] += ig.uth[0] * n[0]; u[1] += ig.uth[1] * n[1]; u[2] += ig.uth[2] * n[2];
    }
    if (ig.gamma_boost > 1.0) {   // :1232-1246 Lorentz transform of the lab-frame density and momentum
        const double gamma_lab = sqrt(1.0 + (u[0] * u[0] + u[1] * u[1] + u[2] * u[2]));
        const double betaz_lab = u[2] / gamma_lab;
        dens = ig.gamma_boost * dens * (1.0 - ig.beta_boost * betaz_lab);
        u[2] = ig.gamma_boost * (u[2] - ig.beta_boost * gamma_lab);
    }
    dst.w[slot] = dens * ig.scale_fac;
    dst.ux[slot] = u[0] * PhysConst::c; dst.uy[slot] = u[1] * PhysConst::c; dst.uz[slot] = u[2] * PhysConst::c;
    if (dst.id) dst.id[slot] = 0;
}

// ---- the injector's constant density: one thread per lattice point ----------------------------------------------
__global__ void __launch_bounds__(256)
add_plasma_kernel(PV dst, InjectGeom ig, long npoints, unsigned long long* __restrict__ count) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = t < npoints;
    double pos[3] = {0.0, 0.0, 0.0};
    if (ok) {
#pragma clang fp contract(off)
        long cell; int iv[3]; double r[3];
        lattice_point(ig, t, cell, iv, r);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            double clo = ig.corner[d] + (iv[d] + 0.0) * ig.dx[d], chi = ig.corner[d] + (iv[d] + 1.0) * ig.dx[d];
            if (d == 2) { clo = ig.gamma_boost * (clo * ig.za - ig.zb); chi = ig.gamma_boost * (chi * ig.za - ig.zb); }   // :1021-1022
            // overlapsWith, and :1030-1048: a corner, an edge midpoint or the centre of the cell has density
            const double mid = (clo + chi) / 2.;
            const bool sample = (clo < ig.hi[d] && clo >= ig.lo[d]) || (mid < ig.hi[d] && mid >= ig.lo[d]) ||
                                (chi < ig.hi[d] && chi >= ig.lo[d]);
            ok = ok && !(clo > ig.hi[d] || chi < ig.lo[d]) && sample;
            pos[d] = ig.corner[d] + (iv[d] + r[d]) * ig.dx[d];                        // getCellCoords
            ok = ok && pos[d] > ig.blo[d] && pos[d] < ig.bhi[d];                      // tile_realbox.contains
            const double lab = d == 2 ? ig.gamma_boost * (pos[d] * ig.za - ig.zb) : pos[d];   // z0 / z0_lab (:1181, :1212)
            ok = ok && lab < ig.hi[d] && lab >= ig.lo[d];                             // insideBounds
        }
    }
    const long slot = inject_slot(ok, dst.np, count);
    if (slot < 0) return;
    double u[3] = {ig.u[0], ig.u[1], ig.u[2]};
    inject_store(dst, ig, slot, pos, u, ig.density);
}

// ---- a density and, optionally, momenta given as expressions --------------------------------------------------
struct InjectProfile {
    const ExprOp* ops;      // ws->inject_prog
    int off[4], n[4];       // 0: the density, 1..3: u_x u_y u_z (in units of c)
    int has_mom;
    double density_min, density_max;
    double ct;              // c t of applyBallisticCorrection
};
// program `which` (wave-uniform) without indexing the kernel argument at run time
__device__ __forceinline__ ExprProg inject_prog(const InjectProfile& pf, int which) {
    const int off = which == 0 ? pf.off[0] : which == 1 ? pf.off[1] : which == 2 ? pf.off[2] : pf.off[3];
    const int n = which == 0 ? pf.n[0] : which == 1 ? pf.n[1] : which == 2 ? pf.n[2] : pf.n[3];
    return ExprProg{pf.ops + off, n};
}
// program `which` at (ax, ay, az)
__device__ __forceinline__ double inject_eval(const InjectProfile& pf, int which, double* col, const double& ax, const double& ay,
                                              const double& az) {
    return expr_run(inject_prog(pf, which), col, [&](int a) { return a == 0 ? ax : (a == 1 ? ay : az); });
}
// applyBallisticCorrection (:138-148) with the bulk momentum u
__device__ __forceinline__ double ballistic_z(double z, double ux, double uy, double uz, double gamma_boost,
                                              double beta_boost, double ct) {
#pragma clang fp contract(off)
    const double gamma_bulk = sqrt(1.0 + (ux * ux + uy * uy + uz * uz));
    const double betaz_bulk = uz / gamma_bulk;
    return gamma_boost * (z * (1.0 - beta_boost * betaz_bulk) - ct * (betaz_bulk - beta_boost));
}

// :1015-1051, one thread per cell: mask[cell] = the cell overlaps the injector's bounds and one of its 27 probe points
// {lo, mid, hi}^3 (z through the ballistic correction) is inside the bounds with a density > 0
__global__ void __launch_bounds__(WXA_EXPR_BLOCK)
add_plasma_probe_kernel(InjectGeom ig, InjectProfile pf, long ncell, unsigned char* __restrict__ mask) {
#pragma clang fp contract(off)
    __shared__ double stack[WXA_EXPR_STACK_DOUBLES];
    double* col = stack + threadIdx.x;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = t < ncell;
    const long cell = live ? t : 0;
    const int i0 = (int)(cell % ig.nc[0]), i1 = (int)((cell / ig.nc[0]) % ig.nc[1]), i2 = (int)(cell / ((long)ig.nc[0] * ig.nc[1]));
    const double lx = ig.corner[0] + (i0 + 0.0) * ig.dx[0], hx = ig.corner[0] + (i0 + 1.0) * ig.dx[0];
    const double ly = ig.corner[1] + (i1 + 0.0) * ig.dx[1], hy = ig.corner[1] + (i1 + 1.0) * ig.dx[1];
    double lz = ig.corner[2] + (i2 + 0.0) * ig.dx[2], hz = ig.corner[2] + (i2 + 1.0) * ig.dx[2];
    if (pf.has_mom) {   // the bulk momentum at the corner that is corrected
        double ul0 = 0., ul1 = 0., ul2 = 0., uh0 = 0., uh1 = 0., uh2 = 0.;
#pragma unroll 1
        for (int k = 0; k < 6; ++k) {
            const bool hi = k >= 3;
            const double ax = hi ? hx : lx, ay = hi ? hy : ly, az = hi ? hz : lz;
            const double r = inject_eval(pf, 1 + k % 3, col, ax, ay, az);
            if (k == 0) ul0 = r; else if (k == 1) ul1 = r; else if (k == 2) ul2 = r;
            else if (k == 3) uh0 = r; else if (k == 4) uh1 = r; else uh2 = r;
        }
        lz = ballistic_z(lz, ul0, ul1, ul2, ig.gamma_boost, ig.beta_boost, pf.ct);
        hz = ballistic_z(hz, uh0, uh1, uh2, ig.gamma_boost, ig.beta_boost, pf.ct);
    } else {
        lz = ig.gamma_boost * (lz * ig.za - ig.zb);
        hz = ig.gamma_boost * (hz * ig.za - ig.zb);
    }
    const bool overlaps = !(lx > ig.hi[0] || hx < ig.lo[0]) && !(ly > ig.hi[1] || hy < ig.lo[1]) && !(lz > ig.hi[2] || hz < ig.lo[2]);
    const double mx = (lx + hx) / 2., my = (ly + hy) / 2., mz = (lz + hz) / 2.;
    bool found = false;
#pragma unroll 1
    for (int k = 0; k < 27; ++k) {
        const int tx = k % 3, ty = (k / 3) % 3, tz = k / 9;
        const double ax = tx == 0 ? lx : (tx == 1 ? mx : hx), ay = ty == 0 ? ly : (ty == 1 ? my : hy),
                     az = tz == 0 ? lz : (tz == 1 ? mz : hz);
        const double dens = inject_eval(pf, 0, col, ax, ay, az);
        const bool inside = ax < ig.hi[0] && ax >= ig.lo[0] && ay < ig.hi[1] && ay >= ig.lo[1] && az < ig.hi[2] && az >= ig.lo[2];
        found = found || (inside && dens > 0);
    }
    if (live) mask[cell] = (overlaps && found) ? 1 : 0;
}

// one thread per lattice point of the cells the probe pass kept (:1175-1276)
__global__ void __launch_bounds__(WXA_EXPR_BLOCK)
add_plasma_profile_kernel(PV dst, InjectGeom ig, InjectProfile pf, long npoints, const unsigned char* __restrict__ mask,
                          unsigned long long* __restrict__ count) {
    __shared__ double stack[WXA_EXPR_STACK_DOUBLES];
    double* col = stack + threadIdx.x;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = t < npoints;
    double pos[3] = {0.0, 0.0, 0.0};
    if (ok) {
#pragma clang fp contract(off)
        long cell; int iv[3]; double r[3];
        lattice_point(ig, t, cell, iv, r);
        ok = mask[cell] != 0;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            pos[d] = ig.corner[d] + (iv[d] + r[d]) * ig.dx[d];                        // getCellCoords
            ok = ok && pos[d] > ig.blo[d] && pos[d] < ig.bhi[d];                      // tile_realbox.contains
        }
    }
    if (!__any(ok)) return;   // nothing of this wave survives the cell tests: no expression is run
    double z0 = 0.0, dens = 0.0, u[3] = {ig.u[0], ig.u[1], ig.u[2]};
    {
#pragma clang fp contract(off)
        if (!pf.has_mom) z0 = ig.gamma_boost * (pos[2] * ig.za - ig.zb);
        double b0 = 0., b1 = 0., b2 = 0.;
        // stages 0..2: the bulk momentum at pos, for z0; 3: the density at (x, y, z0); 4..6: u at (x, y, z0), in a
        // boosted frame at (x, y, 0) (:1239)
#pragma unroll 1
        for (int k = pf.has_mom ? 0 : 3; k < (pf.has_mom ? 7 : 4); ++k) {
            if (k == 3 && pf.has_mom) z0 = ballistic_z(pos[2], b0, b1, b2, ig.gamma_boost, ig.beta_boost, pf.ct);
            const double az = k < 3 ? pos[2] : (k == 3 || !(ig.gamma_boost > 1.0) ? z0 : 0.0);
            const double r = inject_eval(pf, k < 3 ? 1 + k : (k == 3 ? 0 : k - 3), col, pos[0], pos[1], az);
            if (k == 0) b0 = r; else if (k == 1) b1 = r; else if (k == 2) b2 = r; else if (k == 3) dens = r;
            else if (k == 4) u[0] = r; else if (k == 5) u[1] = r; else u[2] = r;
        }
    }
    ok = ok && pos[0] < ig.hi[0] && pos[0] >= ig.lo[0] && pos[1] < ig.hi[1] && pos[1] >= ig.lo[1] && z0 < ig.hi[2] &&
         z0 >= ig.lo[2];                                                              // insideBounds
    ok = ok && !(dens < pf.density_min);
    dens = pf.density_max < dens ? pf.density_max : dens;                             // amrex::min(dens, density_max)
    const long slot = inject_slot(ok, dst.np, count);
    if (slot < 0) return;
    inject_store(dst, ig, slot, pos, u, dens);
}

// one program at n points: vals[v * n + i] = variable v at point i
__global__ void __launch_bounds__(WXA_EXPR_BLOCK)
expr_eval_kernel(ExprProg prog, const double* __restrict__ vals, long n, double* __restrict__ out) {
    __shared__ double stack[WXA_EXPR_STACK_DOUBLES];
    double* col = stack + threadIdx.x;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = t < n;
    const double r = expr_run(prog, col, [&](int a) { return live ? vals[(long)a * n + t] : 0.0; });
    if (live) out[t] = r;
}

// ---- host side of the two injection entries -----------------------------------------------------------------
// The checks both entries make, then the geometry from the arguments; ncell = cells of the box, npoints = lattice points.
static wxa_status inject_setup(const wxa_particle_view* dst, const wxa_plasma_injector* inj, const double corner[3],
                               const int32_t ncells[3], const double dx[3], const double brick_lo[3], const double brick_hi[3],
                               const wxa_injected_momentum* mom, int64_t* n_added, const wxa_workspace* ws, InjectGeom& ig,
                               long& ncell, long& npoints) {
    WXA_REQUIRE(dst && inj && corner && ncells && dx && brick_lo && brick_hi && n_added && ws, "null argument");
    WXA_REQUIRE(pv_ok(dst), "bad particle view");
    WXA_REQUIRE(inj->ppc[0] >= 1 && inj->ppc[1] >= 1 && inj->ppc[2] >= 1, "bad injector");
    *n_added = 0;
    ncell = 1;
    for (int d = 0; d < 3; ++d) {
        WXA_REQUIRE(ncells[d] >= 0 && dx[d] > 0, "bad cell box");
        ig.corner[d] = corner[d]; ig.dx[d] = dx[d]; ig.blo[d] = brick_lo[d]; ig.bhi[d] = brick_hi[d];
        ig.lo[d] = inj->lo[d]; ig.hi[d] = inj->hi[d]; ig.nc[d] = ncells[d]; ig.ppc[d] = inj->ppc[d];
        ig.u[d] = mom ? mom->u_mean[d] : 0.0;
        ig.uth[d] = mom ? mom->u_th[d] : 0.0;
        ig.origin[d] = mom ? mom->origin[d] : 0.0;
        ncell *= ncells[d];
    }
    npoints = ncell * ((long)inj->ppc[0] * inj->ppc[1] * inj->ppc[2]);
    ig.seed = mom ? mom->seed : 0;
    ig.thermal = mom && (mom->u_th[0] != 0.0 || mom->u_th[1] != 0.0 || mom->u_th[2] != 0.0);
    ig.density = inj->density;
    ig.scale_fac = dx[0] * dx[1] * dx[2] / (inj->ppc[0] * inj->ppc[1] * inj->ppc[2]);   // compute_scale_fac_volume
    ig.gamma_boost = inj->gamma_boost > 1.0 ? inj->gamma_boost : 1.0;
    ig.beta_boost = ig.gamma_boost > 1.0 ? std::sqrt(1.0 - 1.0 / std::pow(ig.gamma_boost, 2.0)) : 0.0;
    const double gamma_bulk = std::sqrt(1.0 + (ig.u[0] * ig.u[0] + ig.u[1] * ig.u[1] + ig.u[2] * ig.u[2]));
    const double betaz_bulk = ig.u[2] / gamma_bulk;
    ig.za = 1.0 - ig.beta_boost * betaz_bulk;
    ig.zb = PhysConst::c * inj->t * (betaz_bulk - ig.beta_boost);
    return WXA_OK;
}

// the device's count of added particles (the CW_INJECT pair of ws->counters), zeroed on the stream
static wxa_status inject_counter(wxa_workspace* ws, hipStream_t st, unsigned long long** dcount) {
    wxa_status rc;
    if ((rc = ws->counters.reserve(COUNTER_BYTES)) != WXA_OK) return rc;
    *dcount = (unsigned long long*)((unsigned*)ws->counters.p + CW_INJECT);
    WXA_HIP_CHECK(hipMemsetAsync(*dcount, 0, sizeof(unsigned long long), st));
    return WXA_OK;
}

// the count once the kernels have run: *n_added, or the error of `entry` when it is more than the room
static wxa_status inject_finish(const unsigned long long* dcount, int64_t room, hipStream_t st, const char* entry,
                                int64_t* n_added) {
    unsigned long long h = 0;
    WXA_HIP_CHECK(hipMemcpyAsync(&h, dcount, sizeof(h), hipMemcpyDeviceToHost, st));
    WXA_HIP_CHECK(hipStreamSynchronize(st));
    if ((int64_t)h > room) {
        set_last_error("%s: not enough room for the injected particles", entry);
        return WXA_ERR_NOMEM;
    }
    *n_added = (int64_t)h;
    return WXA_OK;
}

}  // namespace wxa

using namespace wxa;

extern "C" {

wxa_status wxa_add_plasma(const wxa_particle_view* dst, const wxa_plasma_injector* inj, const double corner[3],
                          const int32_t ncells[3], const double dx[3], const double brick_lo[3],
                          const double brick_hi[3], const wxa_injected_momentum* mom, int64_t* n_added,
                          wxa_workspace* ws, void* stream) {
    WXA_REQUIRE(!inj || inj->density >= 0.0, "bad injector");
    InjectGeom ig;
    long ncell, npoints;
    wxa_status rc;
    if ((rc = inject_setup(dst, inj, corner, ncells, dx, brick_lo, brick_hi, mom, n_added, ws, ig, ncell, npoints)) != WXA_OK)
        return rc;
    if (npoints == 0 || !(inj->density > 0)) return WXA_OK;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* dcount;
    if ((rc = inject_counter(ws, st, &dcount)) != WXA_OK) return rc;
    hipLaunchKernelGGL(add_plasma_kernel, dim3(blocks_for(npoints)), dim3(256), 0, st, make_pv(*dst), ig, npoints, dcount);
    WXA_LAUNCH_CHECK();
    return inject_finish(dcount, dst->np, st, "wxa_add_plasma", n_added);
}

wxa_status wxa_expr_compile(const char* text, const char* const* var_names, int32_t nvars, const char* const* const_names,
                            const double* const_values, int32_t nconst, wxa_expr** out) {
    WXA_REQUIRE(text && out && nvars >= 0 && nconst >= 0 && (nvars == 0 || var_names) &&
                (nconst == 0 || (const_names && const_values)), "null argument");
    *out = nullptr;
    try {
        std::vector<std::string> vars;
        std::map<std::string, double> consts;
        for (int i = 0; i < nvars; ++i) { WXA_REQUIRE(var_names[i], "null variable name"); vars.emplace_back(var_names[i]); }
        for (int i = 0; i < nconst; ++i) { WXA_REQUIRE(const_names[i], "null constant name"); consts[const_names[i]] = const_values[i]; }
        *out = new wxa_expr(host::Parser(text, vars, consts));
    } catch (const std::exception& e) {
        set_last_error("wxa_expr_compile: %s", e.what());
        return WXA_ERR_INVALID_ARG;
    }
    return WXA_OK;
}

void wxa_expr_destroy(wxa_expr* e) { delete e; }

wxa_status wxa_expr_eval_host(const wxa_expr* e, const double* vals, double* out) {
    WXA_REQUIRE(e && out && (vals || e->parser.num_vars() == 0), "null argument");
    *out = e->parser.eval(vals);
    return WXA_OK;
}

wxa_status wxa_expr_info(const wxa_expr* e, int32_t* num_ops, int32_t* depth) {
    WXA_REQUIRE(e, "null argument");
    if (num_ops) *num_ops = (int32_t)e->parser.program().size();
    if (depth) *depth = (int32_t)e->parser.depth();
    return WXA_OK;
}

wxa_status wxa_expr_eval_device(wxa_expr* e, const double* vals, int64_t n, double* out, void* stream) {
    WXA_REQUIRE(e && n >= 0 && (n == 0 || out) && (n == 0 || vals || e->parser.num_vars() == 0), "null argument");
    if (!expr_fits_device(e, "wxa_expr_eval_device", "the expression")) return WXA_ERR_INVALID_ARG;
    if (n == 0) return WXA_OK;
    const size_t nops = e->parser.program().size();
    if (!e->dev) {   // uploaded once per expression
        std::vector<ExprOp> ops;
        expr_serialise(e, ops);
        void* d = nullptr;
        WXA_HIP_CHECK(hipMalloc(&d, nops * sizeof(ExprOp)));
        e->dev = d;
        e->dev_free = [](void* q) { (void)hipFree(q); };
        WXA_HIP_CHECK(hipMemcpy(d, ops.data(), nops * sizeof(ExprOp), hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(expr_eval_kernel, dim3(blocks_for(n, WXA_EXPR_BLOCK)), dim3(WXA_EXPR_BLOCK), 0, (hipStream_t)stream,
                       ExprProg{(const ExprOp*)e->dev, (int)nops}, vals, (long)n, out);
    WXA_LAUNCH_CHECK();
    return WXA_OK;
}

wxa_status wxa_workspace_set_injection_profile(wxa_workspace* ws, const wxa_expr* density, const wxa_expr* const* momentum) {
    WXA_REQUIRE(ws && density, "null argument");
    const wxa_expr* e[4] = {density, momentum ? momentum[0] : nullptr, momentum ? momentum[1] : nullptr,
                            momentum ? momentum[2] : nullptr};
    static const char* const what[4] = {"the density expression", "the momentum expression of u_x",
                                        "the momentum expression of u_y", "the momentum expression of u_z"};
    for (int k = 0; k < 4; ++k) {
        if (k > 0 && !momentum) break;
        WXA_REQUIRE(e[k], "null momentum expression");
        WXA_REQUIRE(e[k]->parser.num_vars() == 3, "the expressions of an injector are functions of (x, y, z)");
        if (!expr_fits_device(e[k], "wxa_workspace_set_injection_profile", what[k])) return WXA_ERR_INVALID_ARG;
    }
    std::vector<ExprOp> ops;
    for (int k = 0; k < 4; ++k) {
        ws->inject_id[k] = 0; ws->inject_off[k] = (int32_t)ops.size(); ws->inject_n[k] = 0;
        if (!e[k]) continue;
        expr_serialise(e[k], ops);
        ws->inject_n[k] = (int32_t)ops.size() - ws->inject_off[k];
    }
    wxa_status rc;
    if ((rc = ws->inject_prog.reserve(ops.size() * sizeof(ExprOp))) != WXA_OK) return rc;
    // the buffer may be in use by an earlier injection on any stream: a blocking copy orders the upload behind it
    WXA_HIP_CHECK(hipDeviceSynchronize());
    WXA_HIP_CHECK(hipMemcpy(ws->inject_prog.p, ops.data(), ops.size() * sizeof(ExprOp), hipMemcpyHostToDevice));
    for (int k = 0; k < 4; ++k) ws->inject_id[k] = e[k] ? e[k]->id : 0;
    return WXA_OK;
}

wxa_status wxa_add_plasma_profile(const wxa_particle_view* dst, const wxa_plasma_injector* inj, const double corner[3],
                                  const int32_t ncells[3], const double dx[3], const double brick_lo[3],
                                  const double brick_hi[3], const wxa_injected_momentum* mom, const wxa_expr* density,
                                  const wxa_expr* const* momentum_exprs, double density_min, double density_max,
                                  int64_t* n_added, wxa_workspace* ws, void* stream) {
    WXA_REQUIRE(density, "null argument");
    WXA_REQUIRE(!(mom && momentum_exprs), "momentum given both as wxa_injected_momentum and as expressions");
    InjectGeom ig;
    long ncell, npoints;
    wxa_status rc;
    if ((rc = inject_setup(dst, inj, corner, ncells, dx, brick_lo, brick_hi, mom, n_added, ws, ig, ncell, npoints)) != WXA_OK)
        return rc;
    // the programs are uploaded when they are set; a caller that did not set them sets them here, once
    bool same = ws->inject_id[0] == density->id;
    for (int d = 0; d < 3 && same; ++d) {
        if (momentum_exprs) same = momentum_exprs[d] && ws->inject_id[1 + d] == momentum_exprs[d]->id;
        else same = ws->inject_id[1 + d] == 0;
    }
    if (!same && (rc = wxa_workspace_set_injection_profile(ws, density, momentum_exprs)) != WXA_OK) return rc;
    if (npoints == 0) return WXA_OK;
    InjectProfile pf;
    pf.ops = (const ExprOp*)ws->inject_prog.p;
    for (int k = 0; k < 4; ++k) { pf.off[k] = ws->inject_off[k]; pf.n[k] = ws->inject_n[k]; }
    pf.has_mom = momentum_exprs ? 1 : 0;
    pf.density_min = density_min; pf.density_max = density_max;
    pf.ct = PhysConst::c * inj->t;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* dcount;
    if ((rc = inject_counter(ws, st, &dcount)) != WXA_OK) return rc;
    if ((rc = ws->inject_mask.reserve((size_t)ncell)) != WXA_OK) return rc;
    hipLaunchKernelGGL(add_plasma_probe_kernel, dim3(blocks_for(ncell, WXA_EXPR_BLOCK)), dim3(WXA_EXPR_BLOCK), 0, st, ig, pf,
                       ncell, (unsigned char*)ws->inject_mask.p);
    WXA_LAUNCH_CHECK();
    hipLaunchKernelGGL(add_plasma_profile_kernel, dim3(blocks_for(npoints, WXA_EXPR_BLOCK)), dim3(WXA_EXPR_BLOCK), 0, st,
                       make_pv(*dst), ig, pf, npoints, (const unsigned char*)ws->inject_mask.p, dcount);
    WXA_LAUNCH_CHECK();
    return inject_finish(dcount, dst->np, st, "wxa_add_plasma_profile", n_added);
}

}  // extern "C"
