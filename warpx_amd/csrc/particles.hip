// Particle kernels for gfx950: gather + push (PushPX / PushP), current and charge
// deposition (global-atomics variants; the LDS-tile variants live in deposit_tile.hip),
// periodic wrap, counting sort by cell.
#include "deposit_body.hpp"
#include <complex>

#include "dispatch.hpp"
#include "gather_body.hpp"
#include "push_sort.hpp"
#include "workspace.hpp"

#include <hipcub/hipcub.hpp>

namespace wxa {

template <int O, int G, int PUSHER, bool MOVE>
__global__ void __launch_bounds__(256)
gather_push_kernel(PV p, DevF Ex, DevF Ey, DevF Ez, DevF Bx, DevF By, DevF Bz, Geom g, double q,
                   double m, double dt, ExtEB ext, PushSort hook) {
    const long ip = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (ip >= p.np) return;
    double xp = p.x[ip], yp = p.y[ip], zp = p.z[ip];
    GatherShapes<O, G> s;
    gather_shapes<O, G>(xp, yp, zp, g, s);
    double Exp, Eyp, Ezp, Bxp, Byp, Bzp;
    gather_global<O, G>(s, Ex, Ey, Ez, Bx, By, Bz, Exp, Eyp, Ezp, Bxp, Byp, Bzp);

    add_external_fields(ext, ip, Exp, Eyp, Ezp, Bxp, Byp, Bzp);
    double ux = p.ux[ip], uy = p.uy[ip], uz = p.uz[ip];
    push_momentum<PUSHER>(ux, uy, uz, Exp, Eyp, Ezp, Bxp, Byp, Bzp, q, m, dt);
    if constexpr (MOVE) {
        update_position(xp, yp, zp, ux, uy, uz, dt);
        if (!push_sort_tail<PUSH_SORT_RUNTIME>(&hook, p, ip, xp, yp, zp, ux, uy, uz)) return;   // written to the sorted tile instead
        p.x[ip] = xp; p.y[ip] = yp; p.z[ip] = zp;
    }
    p.ux[ip] = ux; p.uy[ip] = uy; p.uz[ip] = uz;
}

// The repeated plasma lens seen by every particle before the push (add_lens_fields, shapes.hpp):
// out[c * stride + ip], c = Ex Ey Bx By
__global__ void __launch_bounds__(256) lens_fields_kernel(PV p, ExtLens L, double* __restrict__ out, long stride) {
    const long ip = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (ip >= p.np) return;
    double Ex = 0., Ey = 0., Bx = 0., By = 0.;
    add_lens_fields(L, p.x[ip], p.y[ip], p.z[ip], p.ux[ip], p.uy[ip], p.uz[ip], Ex, Ey, Bx, By);
    out[ip] = Ex; out[stride + ip] = Ey; out[2 * stride + ip] = Bx; out[3 * stride + ip] = By;
}

// ---------------------------------------------------------------------------
// One lane per particle, global fp64 atomics (the reference's GPU strategy,
// Source/Particles/Deposition/CurrentDeposition.H:309-334,683-824); used when no cell sort
// is available.  Bodies in deposit_body.hpp.
template <int O>
__global__ void __launch_bounds__(256)
deposit_esirkepov_global_kernel(PV p, DevF Jx, DevF Jy, DevF Jz, Geom g, double q, EsirkepovStep es) {
    const long ip = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (ip >= p.np) return;
    const ParticleState ps{p.x[ip], p.y[ip], p.z[ip], p.w[ip], p.ux[ip], p.uy[ip], p.uz[ip]};
    EsirkepovShapes<O> s;
    esirkepov_shapes<O>(ps, g, q, es, s);
    GlobalSink sink = make_global_sink(Jx, Jy, Jz);
    sink.bi = s.bi; sink.bj = s.bj; sink.bk = s.bk;
    esirkepov_accumulate<O>(s, es, sink);
}

template <int O>
__global__ void __launch_bounds__(256)
deposit_direct_global_kernel(PV p, DevF Jx, DevF Jy, DevF Jz, Geom g, double q, double relative_time) {
    const long ip = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (ip >= p.np) return;
    const ParticleState ps{p.x[ip], p.y[ip], p.z[ip], p.w[ip], p.ux[ip], p.uy[ip], p.uz[ip]};
    DirectShapes<O> s;
    direct_shapes<O>(ps, g, q, relative_time, s);
    GlobalSink sink = make_global_sink(Jx, Jy, Jz);
    direct_accumulate<O>(s, sink);
}

// Source/Particles/Deposition/ChargeDeposition.H:37-180 (3-D), rho of any staggering
template <int O>
__global__ void __launch_bounds__(256)
deposit_charge_kernel(PV p, DevF rho, int s0, int s1, int s2, Geom g, double q) {
    const long ip = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (ip >= p.np) return;
    const double invvol = g.dxi * g.dyi * g.dzi;
    const double wq = q * p.w[ip] * invvol;
    const double x = (p.x[ip] - g.xmin) * g.dxi;
    const double y = (p.y[ip] - g.ymin) * g.dyi;
    const double z = (p.z[ip] - g.zmin) * g.dzi;
    double sx[O + 1], sy[O + 1], sz[O + 1];
    const int i = g.lo0 + shape_factor<O>(sx, s0 ? x : x - 0.5);
    const int j = g.lo1 + shape_factor<O>(sy, s1 ? y : y - 0.5);
    const int k = g.lo2 + shape_factor<O>(sz, s2 ? z : z - 0.5);
    double* __restrict__ r = rho.p + rho.off(i, j, k);
#pragma unroll
    for (int iz = 0; iz <= O; iz++)
#pragma unroll
        for (int iy = 0; iy <= O; iy++)
#pragma unroll
            for (int ix = 0; ix <= O; ix++)
                atomic_add_f64(r + ix + iy * rho.js + iz * rho.ks, sx[ix] * sy[iy] * sz[iz] * wq);
}

__device__ __forceinline__ double wrap_periodic(double v, double plo, double phi) {
    const double L = phi - plo;
    if (v >= phi) {
        v -= L;
        if (v < plo) v = plo;
    } else if (v < plo) {
        v += L;
        if (v >= phi) v = nextafter(phi, plo);
    }
    return v;
}

struct PeriodicBox {
    double plo[3], phi[3];
    int on[3];
};

__global__ void __launch_bounds__(256)
enforce_periodic_kernel(double* __restrict__ x, double* __restrict__ y, double* __restrict__ z, long np,
                        PeriodicBox pb) {
    const long ip = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (ip >= np) return;
    // the three loads first: a conditional store between them would keep one load in flight at a time
    const double vx = pb.on[0] ? x[ip] : 0.0, vy = pb.on[1] ? y[ip] : 0.0, vz = pb.on[2] ? z[ip] : 0.0;
    if (pb.on[0]) { const double w = wrap_periodic(vx, pb.plo[0], pb.phi[0]); if (w != vx) x[ip] = w; }
    if (pb.on[1]) { const double w = wrap_periodic(vy, pb.plo[1], pb.phi[1]); if (w != vy) y[ip] = w; }
    if (pb.on[2]) { const double w = wrap_periodic(vz, pb.plo[2], pb.phi[2]); if (w != vz) z[ip] = w; }
}

// ---- counting sort by cell (the key: SortGeom, cell_of in push_sort.hpp) ---------------
// Histogram + rank.  The input is usually almost sorted (a few % of the particles changed cell
// since the last sort), so equal keys sit in neighbouring lanes: each run of equal keys inside a
// wave issues ONE atomic for the whole run instead of one per particle.
__global__ void __launch_bounds__(256)
sort_count_kernel(const double* __restrict__ x, const double* __restrict__ y,
                  const double* __restrict__ z, const uint64_t* __restrict__ id, long np, SortGeom s,
                  int* __restrict__ cell, int* __restrict__ rank, int* __restrict__ hist) {
    const long ip = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool valid = ip < np;
    const uint64_t pid = (valid && id) ? id[ip] : 0;   // in flight together with the position
    int c = valid ? cell_of(s, x[ip], y[ip], z[ip]) : -1;
    if (valid && id && pid == WXA_IDCPU_RETIRED) c = s.retired_bin;
    const int prev = __shfl_up(c, 1);
    const bool head = (lane == 0) || (c != prev);
    const unsigned long long heads = __ballot(head);
    const unsigned long long upto = (2ULL << lane) - 1ULL;          // bits 0..lane (all ones at lane 63)
    const int hl = 63 - __clzll(heads & upto);                      // head lane of my run
    const unsigned long long above = heads & ~upto;
    const int nh = above ? (__ffsll((long long)above) - 1) : 64;    // first lane of the next run
    int base = 0;
    if (head && c >= 0) base = atomicAdd(&hist[c], nh - lane);
    base = __shfl(base, hl);
    if (valid) {
        if (cell) cell[ip] = c;   // null: the scatter works the key out again from the position it loads anyway
        rank[ip] = base + (lane - hl);
    }
}

// The scatter, for an input that is nearly sorted already (every sort after the first: a particle moves less than
// a cell between sorts, so its destination index is within a few hundred of its source index).  A workgroup takes
// SW_CHUNK consecutive source particles and a window of destination indices around them; a component at a time, the
// particles whose destination lies inside the window are placed at their destination offset in LDS and the window is
// written out in index order -- whole lines instead of 8-byte writes scattered over them -- and the others (movers
// beyond the margin; everything, on an unsorted input) are written directly as before.  A destination slot belongs to
// exactly one particle, so the masked window writes of neighbouring workgroups never touch the same element.
constexpr int SW_THREADS = 512;

// RECELL: the keys are not read from the array the count pass wrote (4 bytes per particle written there and read here, of
// the 152 the sort moves per particle) but worked out again from the position, which this kernel loads anyway: x, y, z and
// the id of the lane's SW_U particles are loaded first and kept for their own component passes.
template <int SW_U, int SW_MARGIN, bool RECELL = false>
__global__ void __launch_bounds__(SW_THREADS)
sort_scatter_window_kernel(PV src, PV dst, const int* __restrict__ cell, const int* __restrict__ rank,
                           const int* __restrict__ offsets, SortGeom sg = SortGeom{}) {
    constexpr int SW_CHUNK = SW_THREADS * SW_U, SW_WIN = SW_CHUNK + 2 * SW_MARGIN;
    __shared__ double win[SW_WIN];
    __shared__ unsigned char mine[SW_WIN];
    const int tid = threadIdx.x;
    const long c0 = (long)blockIdx.x * SW_CHUNK;
    const long w0 = c0 > SW_MARGIN ? c0 - SW_MARGIN : 0;
    for (int a = tid; a < SW_WIN; a += SW_THREADS) mine[a] = 0;
    long d[SW_U];
    int slot[SW_U];   // offset in the window, or -1: written directly
    int ce[SW_U], ra[SW_U];
    double keep[RECELL ? 4 : 1][SW_U];   // RECELL: x, y, z, id (as a bit pattern) of the lane's particles
#pragma unroll
    for (int u = 0; u < SW_U; ++u) {
        const long ip = c0 + u * SW_THREADS + tid;
        const bool in = ip < src.np;
        if constexpr (RECELL) {
            keep[0][u] = in ? src.x[ip] : 0.0; keep[1][u] = in ? src.y[ip] : 0.0; keep[2][u] = in ? src.z[ip] : 0.0;
            keep[3][u] = in && src.id ? reinterpret_cast<const double*>(src.id)[ip] : 0.0;
        } else {
            ce[u] = in ? cell[ip] : 0;
        }
        ra[u] = in ? rank[ip] : 0;
    }
    if constexpr (RECELL) {
#pragma unroll
        for (int u = 0; u < SW_U; ++u) {
            ce[u] = cell_of(sg, keep[0][u], keep[1][u], keep[2][u]);
            if (src.id && __builtin_bit_cast(unsigned long long, keep[3][u]) == WXA_IDCPU_RETIRED) ce[u] = sg.retired_bin;
        }
    }
#pragma unroll
    for (int u = 0; u < SW_U; ++u) {
        const long ip = c0 + u * SW_THREADS + tid;
        d[u] = ip < src.np ? (long)offsets[ce[u]] + ra[u] : -1;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < SW_U; ++u) {
        const long o = d[u] - w0;
        slot[u] = (d[u] >= 0 && o >= 0 && o < SW_WIN) ? (int)o : -1;
        if (slot[u] >= 0) mine[slot[u]] = 1;
    }
    __syncthreads();
    const bool has_id = src.id && dst.id;
    const double* sp[8] = {src.x, src.y, src.z, src.w, src.ux, src.uy, src.uz, reinterpret_cast<const double*>(src.id)};
    double* dp[8] = {dst.x, dst.y, dst.z, dst.w, dst.ux, dst.uy, dst.uz, reinterpret_cast<double*>(dst.id)};
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        if (c == 7 && !has_id) break;
        double v[SW_U];
#pragma unroll
        for (int u = 0; u < SW_U; ++u) {
            const long ip = c0 + u * SW_THREADS + tid;
            if (RECELL && (c < 3 || c == 7)) v[u] = keep[c < 3 ? c : 3][u];
            else v[u] = ip < src.np ? sp[c][ip] : 0.0;   // ids travel as bit patterns
        }
#pragma unroll
        for (int u = 0; u < SW_U; ++u) {
            if (slot[u] >= 0) win[slot[u]] = v[u];
            else if (d[u] >= 0) dp[c][d[u]] = v[u];
        }
        __syncthreads();
        for (int a = tid; a < SW_WIN; a += SW_THREADS)
            if (mine[a]) dp[c][w0 + a] = win[a];
        __syncthreads();
    }
}

// ---- 3-way partition for Redistribute ---------------------------------------------
__global__ void __launch_bounds__(256)
partition_flag_kernel(const double* __restrict__ pos, long np, double lo, double hi, int* __restrict__ stay,
                      unsigned long long* __restrict__ counters) {
    const long ip = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (ip >= np) return;
    const double v = pos[ip];
    const int key = v < lo ? 1 : (v >= hi ? 2 : 0);
    stay[ip] = key == 0 ? 1 : 0;
    if (key) atomicAdd(&counters[key], 1ULL);
}

__global__ void __launch_bounds__(256)
partition_scatter_kernel(PV src, PV dst, const double* __restrict__ pos, double lo, double hi,
                         const int* __restrict__ stay_scan, long nstay, long nminus,
                         unsigned long long* __restrict__ cursors) {
    const long ip = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (ip >= src.np) return;
    const double v = pos[ip];
    long d;
    if (v < lo) d = nstay + (long)atomicAdd(&cursors[1], 1ULL);
    else if (v >= hi) d = nstay + nminus + (long)atomicAdd(&cursors[2], 1ULL);
    else d = stay_scan[ip];
    const double x = src.x[ip], y = src.y[ip], z = src.z[ip], w = src.w[ip];   // every load before the first store
    const double ux = src.ux[ip], uy = src.uy[ip], uz = src.uz[ip];
    const bool has_id = src.id && dst.id;
    const uint64_t id = has_id ? src.id[ip] : 0;
    dst.x[d] = x; dst.y[d] = y; dst.z[d] = z; dst.w[d] = w;
    dst.ux[d] = ux; dst.uy[d] = uy; dst.uz[d] = uz;
    if (has_id) dst.id[d] = id;
}

static inline wxa_particle_view tail_view(const wxa_particle_view& p, int64_t first) {
    wxa_particle_view t = p;
    t.x += first; t.y += first; t.z += first; t.w += first; t.ux += first; t.uy += first; t.uz += first;
    if (t.idcpu) t.idcpu += first;
    t.np = p.np - first;
    return t;
}

// p as the LDS-tile kernels and the global-memory kernels share it: `head`, the particles of the last cell sort (empty
// without a valid one: sorted_tiles_available), on the tiles, and `rest`, those appended since (arrivals from the
// neighbouring bricks; everything without a valid sort), which start `first` particles into p
struct HeadAndRest {
    wxa_particle_view head, rest;
    int64_t first;
};
static inline HeadAndRest split_at_sort(const wxa_workspace* ws, const wxa_particle_view& p) {
    const int64_t first = sorted_tiles_available(ws, &p) ? ws->sorted.np : 0;
    HeadAndRest s{p, tail_view(p, first), first};
    s.head.np = first;
    return s;
}

// ---- laser antenna push (LaserParticleContainer.cpp:795-951, LaserProfileGaussian.cpp:104-161) -------------
// Everything that does not depend on the particle is folded on the host into a complex prefactor
// P = e_max exp(i phase) / D * exp(-(t - t_peak)^2 / tau^2) and the complex inverse waist 1 / (w^2 D),
// D = 1 + 2 i f / (k0 w^2); the amplitude at (X, Y) is Re[P exp(-(X^2 + Y^2) / (w^2 D))].
struct LaserPushGeom {
    double position[3], p_X[3], p_Y[3];
    double mobility;
    double pre_re, pre_im;     // P
    double iw2_re, iw2_im;     // 1 / (w^2 D)
    double drift[3];           // c beta_boost nvec (0 in the lab frame)
    double gamma_boost;        // >= 1
};

__global__ void __launch_bounds__(256)
laser_push_kernel(PV p, LaserPushGeom lg, double dt) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.np) return;
    const double x = p.x[i], y = p.y[i], z = p.z[i];
    const double Xp = lg.p_X[0] * (x - lg.position[0]) + lg.p_X[1] * (y - lg.position[1]) + lg.p_X[2] * (z - lg.position[2]);
    const double Yp = lg.p_Y[0] * (x - lg.position[0]) + lg.p_Y[1] * (y - lg.position[1]) + lg.p_Y[2] * (z - lg.position[2]);
    const double r2 = Xp * Xp + Yp * Yp;
    // exp(-(r2) (a + i b)) = exp(-r2 a) (cos(r2 b) - i sin(r2 b))
    const double mag = exp(-r2 * lg.iw2_re);
    const double er = mag * cos(r2 * lg.iw2_im), ei = -mag * sin(r2 * lg.iw2_im);
    const double amplitude = lg.pre_re * er - lg.pre_im * ei;
    const double sign_charge = (p.w[i] > 0) ? -1.0 : 1.0;
    const double v_over_c = sign_charge * lg.mobility * amplitude;
    // in a boosted frame the antenna also drifts with -beta_boost c along nvec (:907-915)
    const double vx = PhysConst::c * v_over_c * lg.p_X[0] - lg.drift[0];
    const double vy = PhysConst::c * v_over_c * lg.p_X[1] - lg.drift[1];
    const double vz = PhysConst::c * v_over_c * lg.p_X[2] - lg.drift[2];
    const double gamma = lg.gamma_boost / sqrt(1.0 - v_over_c * v_over_c);
    p.ux[i] = gamma * vx; p.uy[i] = gamma * vy; p.uz[i] = gamma * vz;
    p.x[i] = x + vx * dt; p.y[i] = y + vy * dt; p.z[i] = z + vz * dt;
}

// ---- particle walls: WarpXParticleContainer::ApplyBoundaryConditions -------------------------------
struct WallGeom {
    double lo[3], hi[3];
    int bc_lo[3], bc_hi[3];   // WXA_PBOUNDARY_*
};

// apply_boundary / apply_boundaries (Source/Particles/ParticleBoundaries_K.H:20-175): beyond a reflecting
// wall the position is mirrored and the normal momentum flips; beyond an absorbing wall the particle is
// lost = retired in place (weight and momentum 0, position clamped into the domain, idcpu marked).
__global__ void __launch_bounds__(256)
particle_walls_kernel(PV p, WallGeom wg, unsigned* __restrict__ n_lost) {
    const long ip = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (ip >= p.np) return;
    double x[3] = {p.x[ip], p.y[ip], p.z[ip]};
    if (p.id[ip] == WXA_IDCPU_RETIRED) {
        // A retired particle stays in the tile until the next sort and is still pushed (weight 0: it deposits
        // nothing): park it inside the domain again and take its momentum away, every step, so that it can never
        // drift out of the range the field arrays cover -- however long the sort is away
        bool out = false;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double c = fmin(fmax(x[d], wg.lo[d]), nextafter(wg.hi[d], wg.lo[d]));
            out = out || c != x[d];
            x[d] = c;
        }
        if (out) { p.x[ip] = x[0]; p.y[ip] = x[1]; p.z[ip] = x[2]; }
        p.ux[ip] = 0.0; p.uy[ip] = 0.0; p.uz[ip] = 0.0;
        return;
    }
    bool lost = false, flip[3] = {false, false, false}, moved = false;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        if (x[d] < wg.lo[d]) {
            if (wg.bc_lo[d] == WXA_PBOUNDARY_ABSORBING) lost = true;
            else if (wg.bc_lo[d] == WXA_PBOUNDARY_REFLECTING) { x[d] = 2 * wg.lo[d] - x[d]; flip[d] = true; moved = true; }
        } else if (x[d] > wg.hi[d]) {
            if (wg.bc_hi[d] == WXA_PBOUNDARY_ABSORBING) lost = true;
            else if (wg.bc_hi[d] == WXA_PBOUNDARY_REFLECTING) { x[d] = 2 * wg.hi[d] - x[d]; flip[d] = true; moved = true; }
        }
    }
    if (lost) {
#pragma unroll
        for (int d = 0; d < 3; ++d) x[d] = fmin(fmax(x[d], wg.lo[d]), nextafter(wg.hi[d], wg.lo[d]));
        p.x[ip] = x[0]; p.y[ip] = x[1]; p.z[ip] = x[2];
        p.w[ip] = 0.0; p.ux[ip] = 0.0; p.uy[ip] = 0.0; p.uz[ip] = 0.0;
        p.id[ip] = WXA_IDCPU_RETIRED;
        atomicAdd(n_lost, 1u);
    } else if (moved) {
        if (flip[0]) { p.x[ip] = x[0]; p.ux[ip] = -p.ux[ip]; }
        if (flip[1]) { p.y[ip] = x[1]; p.uy[ip] = -p.uy[ip]; }
        if (flip[2]) { p.z[ip] = x[2]; p.uz[ip] = -p.uz[ip]; }
    }
}

// ---- Redistribute without moving the tile (see include/warpx_amd.h) --------------------
struct ClassifyGeom {
    double plo[3], phi[3], blo[3], bhi[3];
    int periodic[3], split[3];
};

// DEST = false: 6 lists, by the first split direction in which the particle is outside (before the wrap);
// DEST = true: 27 lists, by the offset of the destination brick (wxa_wrap_and_classify_dest)
template <bool DEST>
__global__ void __launch_bounds__(256)
wrap_classify_kernel(double* __restrict__ x, double* __restrict__ y, double* __restrict__ z,
                     const uint64_t* __restrict__ id, long first, long count, ClassifyGeom cg,
                     int* __restrict__ lists, long cap, unsigned* __restrict__ counts) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const long ip = first + t;
    double v[3] = {x[ip], y[ip], z[ip]};
    int code = -1;
    if constexpr (DEST) {
        int o[3] = {0, 0, 0};
#pragma unroll
        for (int d = 0; d < 3; ++d)
            if (cg.split[d]) o[d] = v[d] < cg.blo[d] ? -1 : (v[d] >= cg.bhi[d] ? 1 : 0);
        code = (o[0] + 1) + 3 * (o[1] + 1) + 9 * (o[2] + 1);
        if (code == 13) code = -1;
    } else {
#pragma unroll
        for (int d = 0; d < 3; ++d)
            if (cg.split[d] && code < 0) code = v[d] < cg.blo[d] ? 2 * d : (v[d] >= cg.bhi[d] ? 2 * d + 1 : -1);
    }
    if (code >= 0 && id[ip] == WXA_IDCPU_RETIRED) {
        // A retired particle is still pushed until the next sort drops it (weight 0: it deposits zeros).  It was
        // parked on the brick's side of the face it left through, so the push can carry it across again; if
        // that face is the domain boundary the periodic wrap would send it a whole domain away, where its
        // stencils lie outside this brick's arrays.  Park it again instead.
        code = -1;
#pragma unroll
        for (int d = 0; d < 3; ++d)
            if (cg.split[d]) v[d] = fmin(fmax(v[d], cg.blo[d]), nextafter(cg.bhi[d], cg.blo[d]));
        if (v[0] != x[ip]) x[ip] = v[0];
        if (v[1] != y[ip]) y[ip] = v[1];
        if (v[2] != z[ip]) z[ip] = v[2];
    }
    if (cg.periodic[0]) { const double w = wrap_periodic(v[0], cg.plo[0], cg.phi[0]); if (w != v[0]) x[ip] = w; }
    if (cg.periodic[1]) { const double w = wrap_periodic(v[1], cg.plo[1], cg.phi[1]); if (w != v[1]) y[ip] = w; }
    if (cg.periodic[2]) { const double w = wrap_periodic(v[2], cg.plo[2], cg.phi[2]); if (w != v[2]) z[ip] = w; }
    if (code >= 0) {
        const unsigned slot = atomicAdd(&counts[code], 1u);
        if ((long)slot < cap) lists[code * cap + slot] = (int)ip;
    }
}

__global__ void __launch_bounds__(256)
pack_leavers_kernel(PV p, const int* __restrict__ list, long n, double* __restrict__ msg, long row_len,
                    long offset, int retire, ClassifyGeom cg) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const long ip = list[t];
    double* m = msg + offset + t;
    m[0 * row_len] = p.x[ip]; m[1 * row_len] = p.y[ip]; m[2 * row_len] = p.z[ip]; m[3 * row_len] = p.w[ip];
    m[4 * row_len] = p.ux[ip]; m[5 * row_len] = p.uy[ip]; m[6 * row_len] = p.uz[ip];
    reinterpret_cast<uint64_t*>(m)[7 * row_len] = p.id[ip];
    if (retire) {
        // inert from here on: deposits exact zeros, stays inside the brick (and inside the reach of
        // its tile), and is dropped by the next sort
        double* pos[3] = {p.x, p.y, p.z};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const double v = pos[d][ip];
            const double inside = fmin(fmax(v, cg.blo[d]), nextafter(cg.bhi[d], cg.blo[d]));
            if (inside != v) pos[d][ip] = inside;
        }
        p.w[ip] = 0.0; p.ux[ip] = 0.0; p.uy[ip] = 0.0; p.uz[ip] = 0.0;
        p.id[ip] = WXA_IDCPU_RETIRED;
    }
}

// per-particle external fields of the push that follows (none unless the workspace carries a lens)
static wxa_status evaluate_particle_fields(const wxa_particle_view* p, wxa_workspace* ws, hipStream_t st) {
    if (!ws) return WXA_OK;
    ws->ext_pp_stride = 0;
    if (ws->lens_n <= 0 || p->np == 0) return WXA_OK;
    wxa_status rc;
    if ((rc = ws->ext_pp.reserve(sizeof(double) * 4 * (size_t)p->np)) != WXA_OK) return rc;
    const PV pv = make_pv(*p);
    hipLaunchKernelGGL(lens_fields_kernel, dim3(blocks_for(pv.np)), dim3(256), 0, st, pv, lens_of(ws), (double*)ws->ext_pp.p,
                       (long)p->np);
    WXA_LAUNCH_CHECK();
    ws->ext_pp_stride = p->np;
    return WXA_OK;
}

static wxa_status check_gather_args(const wxa_particle_view* p, const wxa_field_view E[3],
                                    const wxa_field_view B[3], const wxa_grid_geom* geom, int order,
                                    int galerkin, int pusher) {
    WXA_REQUIRE(pv_ok(p), "bad particle view");
    WXA_REQUIRE(E && B && geom, "null argument");
    for (int c = 0; c < 3; ++c) WXA_REQUIRE(view_ok(E[c]) && view_ok(B[c]), "bad field view");
    WXA_REQUIRE(order >= 1 && order <= 4, "particle shape order must be 1..4");
    WXA_REQUIRE(galerkin == 0 || galerkin == 1, "galerkin must be 0 or 1");
    WXA_REQUIRE(pusher >= WXA_PUSHER_BORIS && pusher <= WXA_PUSHER_BORIS_RR,
                "pusher must be Boris, Vay, Higuera-Cary or Boris with radiation reaction");
    if (!yee_E(E) || !yee_B(B)) {
        set_last_error("gather: only the Yee staggering is supported");
        return WXA_ERR_UNSUPPORTED;
    }
    return WXA_OK;
}

// out[i] = in[0] + ... + in[i - 1], i < n (hipCUB; its temporary storage is ws->scan_tmp)
static wxa_status exclusive_scan(int* in, int* out, int n, wxa_workspace* ws, hipStream_t st) {
    size_t tmp_bytes = 0;
    WXA_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, in, out, n, st));
    if (const wxa_status rc = ws->scan_tmp.reserve(tmp_bytes); rc != WXA_OK) return rc;
    WXA_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(ws->scan_tmp.p, tmp_bytes, in, out, n, st));
    return WXA_OK;
}

// the box of a periodic wrap; any: some direction is periodic (none: there is nothing to wrap)
static wxa_status make_periodic_box(const double plo[3], const double phi[3], const int periodic[3], PeriodicBox& pb, bool& any) {
    any = false;
    for (int d = 0; d < 3; ++d) {
        pb.plo[d] = plo[d]; pb.phi[d] = phi[d]; pb.on[d] = periodic[d] ? 1 : 0;
        if (periodic[d]) { WXA_REQUIRE(phi[d] > plo[d], "empty domain"); any = true; }
    }
    return WXA_OK;
}

}  // namespace wxa

using namespace wxa;

extern "C" {

// the global-memory kernel on `rest` with the external fields `ext`
static wxa_status gather_push_global(const wxa_particle_view& rest, const wxa_field_view E[3], const wxa_field_view B[3],
                                     const wxa_grid_geom* geom, double q, double m, double dt, int order, int galerkin,
                                     int pusher, int move, const ExtEB& ext, const PushSort& hook, hipStream_t st) {
    const PV pv = make_pv(rest);
    const Geom g = make_geom(*geom);
    const DevF ex = make_devf(E[0]), ey = make_devf(E[1]), ez = make_devf(E[2]);
    const DevF bx = make_devf(B[0]), by = make_devf(B[1]), bz = make_devf(B[2]);
    with_int<WXA_PUSHER_BORIS, WXA_PUSHER_VAY, WXA_PUSHER_HC, WXA_PUSHER_BORIS_RR>(pusher, [&](auto pu) {
    with_int<1, 0>(move != 0, [&](auto mv) {
    with_int<1, 2, 3, 4>(order, [&](auto o) {
    with_int<1, 0>(galerkin, [&](auto gk) {
        hipLaunchKernelGGL((gather_push_kernel<decltype(o)::value, decltype(gk)::value, decltype(pu)::value, decltype(mv)::value != 0>),
                           dim3(blocks_for(pv.np)), dim3(256), 0, st, pv, ex, ey, ez, bx, by, bz, g, q, m, dt, ext, hook);
    }); }); }); });
    WXA_LAUNCH_CHECK();
    return WXA_OK;
}

wxa_status wxa_gather_push_ws(const wxa_particle_view* p, const wxa_field_view E[3], const wxa_field_view B[3],
                              const wxa_grid_geom* geom, double q, double m, double dt, int order, int galerkin,
                              int pusher, int move, wxa_workspace* ws, void* stream) {
    wxa_status rc = check_gather_args(p, E, B, geom, order, galerkin, pusher);
    if (rc != WXA_OK) return rc;
    if (p->np == 0) return WXA_OK;
    if ((rc = evaluate_particle_fields(p, ws, (hipStream_t)stream)) != WXA_OK) return rc;
    // sorted part on the LDS tiles (orders 1 .. 4; 4 since round 6: a tile of 13^3 / 14^3 staged points); particles
    // appended since the sort (arrivals from the neighbouring bricks) take the global-memory kernel below
    const HeadAndRest s = split_at_sort(ws, *p);
    if (s.head.np > 0 &&
        (rc = gather_push_tiled(&s.head, E, B, geom, q, m, dt, order, galerkin, pusher, move != 0, 0, ws,
                                (hipStream_t)stream)) != WXA_OK)
        return rc;
    if (s.rest.np == 0) return WXA_OK;
    return gather_push_global(s.rest, E, B, geom, q, m, dt, order, galerkin, pusher, move, ext_of(ws, s.first),
                              make_push_sort(ws, s.first, move != 0), (hipStream_t)stream);
}

wxa_status wxa_gather_push_part(const wxa_particle_view* p, const wxa_field_view E[3], const wxa_field_view B[3],
                                const wxa_grid_geom* geom, double q, double m, double dt, int order, int galerkin,
                                int pusher, wxa_workspace* ws, int part, void* stream) {
    wxa_status rc = check_gather_args(p, E, B, geom, order, galerkin, pusher);
    if (rc != WXA_OK) return rc;
    WXA_REQUIRE(part == WXA_PART_INTERIOR || part == WXA_PART_REST, "part must be WXA_PART_INTERIOR or WXA_PART_REST");
    if (p->np == 0) return WXA_OK;
    if ((rc = evaluate_particle_fields(p, ws, (hipStream_t)stream)) != WXA_OK) return rc;
    const HeadAndRest s = split_at_sort(ws, *p);   // no tiles: the interior part is empty, the rest is everything
    if (s.head.np > 0 &&
        (rc = gather_push_tiled(&s.head, E, B, geom, q, m, dt, order, galerkin, pusher, true, part, ws,
                                (hipStream_t)stream)) != WXA_OK)
        return rc;
    if (part == WXA_PART_INTERIOR || s.rest.np == 0) return WXA_OK;   // arrivals since the sort may sit anywhere
    return gather_push_global(s.rest, E, B, geom, q, m, dt, order, galerkin, pusher, 1, ext_of(ws, s.first),
                              make_push_sort(ws, s.first, true), (hipStream_t)stream);
}

wxa_status wxa_gather_push(const wxa_particle_view* p, const wxa_field_view E[3], const wxa_field_view B[3],
                           const wxa_grid_geom* geom, double q, double m, double dt, int order, int galerkin,
                           int pusher, void* stream) {
    return wxa_gather_push_ws(p, E, B, geom, q, m, dt, order, galerkin, pusher, 1, nullptr, stream);
}

wxa_status wxa_push_p(const wxa_particle_view* p, const wxa_field_view E[3], const wxa_field_view B[3],
                      const wxa_grid_geom* geom, double q, double m, double dt, int order, int galerkin,
                      int pusher, void* stream) {
    return wxa_gather_push_ws(p, E, B, geom, q, m, dt, order, galerkin, pusher, 0, nullptr, stream);
}

wxa_status wxa_deposit_current(const wxa_particle_view* p, const wxa_field_view J[3], const wxa_grid_geom* geom,
                               double q, double dt, double relative_time, int order, int algo,
                               wxa_workspace* ws, void* stream) {
    WXA_REQUIRE(pv_ok(p), "bad particle view");
    WXA_REQUIRE(J && geom, "null argument");
    for (int c = 0; c < 3; ++c) WXA_REQUIRE(view_ok(J[c]), "bad field view");
    WXA_REQUIRE(order >= 1 && order <= 4, "particle shape order must be 1..4");
    WXA_REQUIRE(algo == WXA_DEPOSIT_ESIRKEPOV || algo == WXA_DEPOSIT_DIRECT, "unknown deposition algorithm");
    WXA_REQUIRE(dt > 0.0 || algo == WXA_DEPOSIT_DIRECT, "dt must be positive");
    if (!yee_E(J)) {
        set_last_error("deposit_current: only the Yee staggering is supported");
        return WXA_ERR_UNSUPPORTED;
    }
    if (p->np == 0) return WXA_OK;
    hipStream_t st = (hipStream_t)stream;
    // sorted part on the LDS tiles (orders 1 .. 4; 4 since round 6: the tile's points are exactly the quartic stencil's
    // reach); arrivals since the sort: global atomics
    const HeadAndRest s = split_at_sort(ws, *p);
    wxa_status rc;
    if (s.head.np > 0 && (rc = deposit_current_tiled(&s.head, J, geom, q, dt, relative_time, order, algo, ws, st)) != WXA_OK)
        return rc;
    if (s.rest.np == 0) return WXA_OK;
    const PV pv = make_pv(s.rest);
    const Geom g = make_geom(*geom);
    const DevF jx = make_devf(J[0]), jy = make_devf(J[1]), jz = make_devf(J[2]);
    const dim3 grid(blocks_for(pv.np)), block(256);
    with_int<1, 2, 3, 4>(order, [&](auto o) {
        constexpr int O = decltype(o)::value;
        if (algo == WXA_DEPOSIT_ESIRKEPOV)
            hipLaunchKernelGGL(deposit_esirkepov_global_kernel<O>, grid, block, 0, st, pv, jx, jy, jz, g, q,
                               make_esirkepov_step(g, dt, relative_time));
        else hipLaunchKernelGGL(deposit_direct_global_kernel<O>, grid, block, 0, st, pv, jx, jy, jz, g, q, relative_time);
    });
    WXA_LAUNCH_CHECK();
    return WXA_OK;
}

wxa_status wxa_deposit_charge(const wxa_particle_view* p, const wxa_field_view* rho, const wxa_grid_geom* geom,
                              double q, int order, void* stream) {
    WXA_REQUIRE(pv_ok(p), "bad particle view");
    WXA_REQUIRE(rho && geom && view_ok(*rho), "bad argument");
    WXA_REQUIRE(order >= 1 && order <= 4, "particle shape order must be 1..4");
    if (p->np == 0) return WXA_OK;
    const PV pv = make_pv(*p);
    const Geom g = make_geom(*geom);
    const DevF r = make_devf(*rho);
    with_int<1, 2, 3, 4>(order, [&](auto o) {
        hipLaunchKernelGGL(deposit_charge_kernel<decltype(o)::value>, dim3(blocks_for(pv.np)), dim3(256), 0, (hipStream_t)stream, pv,
                           r, rho->stag[0], rho->stag[1], rho->stag[2], g, q);
    });
    WXA_LAUNCH_CHECK();
    return WXA_OK;
}

wxa_status wxa_enforce_periodic(const wxa_particle_view* p, const double plo[3], const double phi[3],
                                const int periodic[3], void* stream) {
    WXA_REQUIRE(pv_ok(p) && plo && phi && periodic, "bad argument");
    if (p->np == 0) return WXA_OK;
    PeriodicBox pb;
    bool any;
    const wxa_status rc = make_periodic_box(plo, phi, periodic, pb, any);
    if (rc != WXA_OK || !any) return rc;
    hipLaunchKernelGGL(enforce_periodic_kernel, dim3(blocks_for(p->np)), dim3(256), 0, (hipStream_t)stream, p->x,
                       p->y, p->z, (long)p->np, pb);
    WXA_LAUNCH_CHECK();
    return WXA_OK;
}

// The periodic wrap restricted to the particles that can need it: those of the tiles of the last cell sort that touch
// a periodic face of the sorted box (= the domain on a single brick), plus the particles appended since.  A particle
// moves less than one cell per step, so while fewer steps than a tile is wide have passed since the sort, a particle
// of an interior tile cannot have left the domain.  Same arithmetic as wxa_enforce_periodic on 18 % of the particles
// (256^3 in tiles of 8^3).
constexpr int EPT_THREADS = 256, EPT_SPLIT = 4;   // four workgroups per tile, x 4 particles per lane: a quarter of a tile of 8 per cell in one pass (per launch, 256^3: 0.300 ms with one workgroup per tile, 0.342 with one of 1024 lanes, 0.172 with four, 0.253 with eight)
__global__ void __launch_bounds__(EPT_THREADS)
enforce_periodic_tiles_kernel(double* __restrict__ x, double* __restrict__ y, double* __restrict__ z,
                              const int* __restrict__ offsets, int nt0, int nt1, int nt2, int nc0, int nc1, int nc2,
                              PeriodicBox pb) {
    constexpr int T = WXA_TILE;
    const int tile = blockIdx.x / EPT_SPLIT, part = blockIdx.x % EPT_SPLIT;
    const int ti = tile % nt0, tj = (tile / nt0) % nt1, tk = tile / (nt0 * nt1);
    // a tile whose cells lie within a tile width of a periodic face (the last tile of a direction may be partial)
    const bool face = (pb.on[0] && (ti == 0 || (ti + 2) * T > nc0)) || (pb.on[1] && (tj == 0 || (tj + 2) * T > nc1)) ||
                      (pb.on[2] && (tk == 0 || (tk + 2) * T > nc2));
    if (!face) return;
    constexpr int TC = WXA_TILE * WXA_TILE * WXA_TILE;
    const int t_start = offsets[(long)tile * TC], t_end = offsets[(long)(tile + 1) * TC];
    const int per = (t_end - t_start + EPT_SPLIT - 1) / EPT_SPLIT;
    const int start = t_start + part * per, end = min(start + per, t_end);
    // four particles per lane and pass, all their loads in flight before the first (conditional) store: written as one
    // load - test - store after the other, the kernel had one load in flight per lane (0.49 ms for 18 % of the particles)
    constexpr int U = 4;
    for (int base = start + (int)threadIdx.x; base < end; base += EPT_THREADS * U) {
        double v[U][3];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int ip = base + u * EPT_THREADS;
            const bool in = ip < end;
            v[u][0] = in && pb.on[0] ? x[ip] : 0.0;
            v[u][1] = in && pb.on[1] ? y[ip] : 0.0;
            v[u][2] = in && pb.on[2] ? z[ip] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int ip = base + u * EPT_THREADS;
            if (ip >= end) continue;
            if (pb.on[0]) { const double w = wrap_periodic(v[u][0], pb.plo[0], pb.phi[0]); if (w != v[u][0]) x[ip] = w; }
            if (pb.on[1]) { const double w = wrap_periodic(v[u][1], pb.plo[1], pb.phi[1]); if (w != v[u][1]) y[ip] = w; }
            if (pb.on[2]) { const double w = wrap_periodic(v[u][2], pb.plo[2], pb.phi[2]); if (w != v[u][2]) z[ip] = w; }
        }
    }
}

wxa_status wxa_enforce_periodic_sorted(const wxa_particle_view* p, const double plo[3], const double phi[3],
                                       const int periodic[3], wxa_workspace* ws, int32_t steps_since_sort,
                                       void* stream) {
    WXA_REQUIRE(pv_ok(p) && plo && phi && periodic, "bad argument");
    // no usable sort, or the drift since it may exceed a tile: the plain pass over everything
    if (!sorted_tiles_available(ws, p) || steps_since_sort < 0 || steps_since_sort > WXA_TILE - 2)
        return wxa_enforce_periodic(p, plo, phi, periodic, stream);
    if (p->np == 0) return WXA_OK;
    PeriodicBox pb;
    bool any;
    const wxa_status rc = make_periodic_box(plo, phi, periodic, pb, any);
    if (rc != WXA_OK || !any) return rc;
    const SortRecord& so = ws->sorted;
    const int nt0 = so.tiles(0), nt1 = so.tiles(1), nt2 = so.tiles(2);
    hipLaunchKernelGGL(enforce_periodic_tiles_kernel, dim3((unsigned)(nt0 * nt1 * nt2) * EPT_SPLIT), dim3(EPT_THREADS), 0, (hipStream_t)stream,
                       p->x, p->y, p->z, (const int*)ws->offsets.p, nt0, nt1, nt2, so.nc[0], so.nc[1], so.nc[2], pb);
    if (p->np > so.np) {   // appended since the sort
        const wxa_particle_view tail = tail_view(*p, so.np);
        hipLaunchKernelGGL(enforce_periodic_kernel, dim3(blocks_for(tail.np)), dim3(256), 0, (hipStream_t)stream,
                           tail.x, tail.y, tail.z, (long)tail.np, pb);
    }
    WXA_LAUNCH_CHECK();
    return WXA_OK;
}

wxa_status wxa_sort_particles_by_cell(const wxa_particle_view* src, const wxa_particle_view* dst,
                                      const double plo[3], const double dinv[3], const int32_t cell_lo[3],
                                      const int32_t ncell[3], wxa_workspace* ws, void* stream) {
    WXA_REQUIRE(pv_ok(src) && pv_ok(dst) && plo && dinv && cell_lo && ncell && ws, "bad argument");
    WXA_REQUIRE(src->np == dst->np, "src/dst particle counts differ");
    WXA_REQUIRE(src->x != dst->x, "sort is out of place");
    WXA_REQUIRE(ncell[0] > 0 && ncell[1] > 0 && ncell[2] > 0, "empty cell box");
    const SortRecord sorted = SortRecord::of(dst->x, src->np, plo, dinv, cell_lo, ncell);   // (np: wxa_sort_live_count lowers it)
    const long ncells = sorted.bins;
    WXA_REQUIRE(ncells > 0 && ncells < (1L << 31) - 2 && src->np < (1L << 31) - 2, "sizes exceed 32-bit sort keys");
    hipStream_t st = (hipStream_t)stream;
    ws->sorted.valid = false;
    ws->ps.pending.valid = false;   // a record of wxa_push_sort_begin(COUNT) indexes the order this sort replaces
    if (src->np == 0) return WXA_OK;
    wxa_status rc;
    if ((rc = ws->rank.reserve(sizeof(int) * src->np)) != WXA_OK) return rc;   // (no key array: the scatter works the keys out again)
    // bins: the cells, the retired particles, and one closing entry for the scan
    if ((rc = ws->hist.reserve(sizeof(int) * (ncells + 2))) != WXA_OK) return rc;
    if ((rc = ws->offsets.reserve(sizeof(int) * (ncells + 2))) != WXA_OK) return rc;
    int* rank = (int*)ws->rank.p;
    int* hist = (int*)ws->hist.p; int* offsets = (int*)ws->offsets.p;
    WXA_HIP_CHECK(hipMemsetAsync(hist, 0, sizeof(int) * (ncells + 2), st));
    const SortGeom sg = sort_geom_of(sorted);
    const PV s = make_pv(*src), d = make_pv(*dst);
    hipLaunchKernelGGL(sort_count_kernel, dim3(blocks_for(s.np)), dim3(256), 0, st, s.x, s.y, s.z, s.id, s.np, sg,
                       (int*)nullptr, rank, hist);
    if ((rc = exclusive_scan(hist, offsets, (int)(ncells + 2), ws, st)) != WXA_OK) return rc;
    // the scatter works the keys out again from the positions it loads (round 4) and stages a chunk's near-stayers in LDS
    // in destination order, so that it writes whole lines.  Window shapes timed at 256^3 x 8 ppc (Redistribute per step;
    // the plain scatter -- one lane per particle, 8-byte writes wherever they fall -- 1.47): 8 x 512 lanes + 512 margin
    // 1.24, 4 x 512 + 512 1.29, 8 x 512 + 1024 1.25, 16 x 512 + 512 1.38
    hipLaunchKernelGGL((sort_scatter_window_kernel<8, 512, true>), dim3(blocks_for(s.np, SW_THREADS * 8)), dim3(SW_THREADS), 0,
                       st, s, d, (const int*)nullptr, rank, offsets, sg);
    WXA_LAUNCH_CHECK();
    ws->sorted = sorted;
    return WXA_OK;
}

wxa_status wxa_partition_particles(const wxa_particle_view* src, const wxa_particle_view* dst, int dim,
                                   double lo, double hi, int64_t counts[3], wxa_workspace* ws, void* stream) {
    WXA_REQUIRE(pv_ok(src) && pv_ok(dst) && counts && ws, "bad argument");
    WXA_REQUIRE(dim >= 0 && dim < 3, "dim must be 0..2");
    WXA_REQUIRE(src->np == dst->np && (src->np == 0 || src->x != dst->x), "partition is out of place, equal sizes");
    WXA_REQUIRE(src->np < (1L << 31) - 2, "tile too large for 32-bit scan");
    hipStream_t st = (hipStream_t)stream;
    counts[0] = counts[1] = counts[2] = 0;
    ws->sorted.valid = false;
    ws->ps.pending.valid = false;
    if (src->np == 0) return WXA_OK;
    wxa_status rc;
    if ((rc = ws->cell.reserve(sizeof(int) * (src->np + 1))) != WXA_OK) return rc;
    if ((rc = ws->rank.reserve(sizeof(int) * (src->np + 1))) != WXA_OK) return rc;
    if ((rc = ws->hist.reserve(sizeof(unsigned long long) * 8)) != WXA_OK) return rc;
    int* stay = (int*)ws->cell.p; int* scan = (int*)ws->rank.p;
    unsigned long long* ctr = (unsigned long long*)ws->hist.p;
    WXA_HIP_CHECK(hipMemsetAsync(ctr, 0, sizeof(unsigned long long) * 8, st));
    const PV s = make_pv(*src), d = make_pv(*dst);
    const double* pos = dim == 0 ? s.x : (dim == 1 ? s.y : s.z);
    hipLaunchKernelGGL(partition_flag_kernel, dim3(blocks_for(s.np)), dim3(256), 0, st, pos, s.np, lo, hi, stay, ctr);
    if ((rc = exclusive_scan(stay, scan, (int)s.np, ws, st)) != WXA_OK) return rc;
    unsigned long long h[3] = {0, 0, 0};
    WXA_HIP_CHECK(hipMemcpyAsync(h, ctr, sizeof(h), hipMemcpyDeviceToHost, st));
    WXA_HIP_CHECK(hipStreamSynchronize(st));
    const long nminus = (long)h[1], nplus = (long)h[2], nstay = s.np - nminus - nplus;
    hipLaunchKernelGGL(partition_scatter_kernel, dim3(blocks_for(s.np)), dim3(256), 0, st, s, d, pos, lo, hi, scan,
                       nstay, nminus, ctr + 3);
    WXA_LAUNCH_CHECK();
    counts[0] = nstay; counts[1] = nminus; counts[2] = nplus;
    return WXA_OK;
}

}  // extern "C"

template <bool DEST>
static wxa_status wrap_and_classify_impl(const wxa_particle_view* p, int64_t first, int64_t count, const double prob_lo[3],
                                         const double prob_hi[3], const int periodic[3], const double brick_lo[3],
                                         const double brick_hi[3], const int split[3], int32_t* lists, int64_t capacity,
                                         int64_t* counts, wxa_workspace* ws, void* stream) {
    constexpr int NL = DEST ? 27 : 6;
    WXA_REQUIRE(pv_ok(p) && prob_lo && prob_hi && periodic && brick_lo && brick_hi && split && counts && ws,
                "bad argument");
    WXA_REQUIRE(first >= 0 && count >= 0 && first + count <= p->np, "range outside the tile");
    WXA_REQUIRE(capacity >= 0 && (capacity == 0 || lists), "null list storage");
    const bool any_split = split[0] || split[1] || split[2];
    WXA_REQUIRE(!any_split || p->idcpu, "idcpu is needed to recognise retired particles");
    for (int c = 0; c < NL; ++c) counts[c] = 0;
    if (count == 0) return WXA_OK;
    ClassifyGeom cg;
    for (int d = 0; d < 3; ++d) {
        cg.plo[d] = prob_lo[d]; cg.phi[d] = prob_hi[d]; cg.blo[d] = brick_lo[d]; cg.bhi[d] = brick_hi[d];
        cg.periodic[d] = periodic[d] ? 1 : 0; cg.split[d] = split[d] ? 1 : 0;
        if (periodic[d]) WXA_REQUIRE(prob_hi[d] > prob_lo[d], "empty domain");
    }
    hipStream_t st = (hipStream_t)stream;
    wxa_status rc;
    if ((rc = ws->counters.reserve(COUNTER_BYTES)) != WXA_OK) return rc;
    unsigned* dcount = (unsigned*)ws->counters.p + (DEST ? CW_DEST : CW_CLASSIFY);
    WXA_HIP_CHECK(hipMemsetAsync(dcount, 0, NL * sizeof(unsigned), st));
    hipLaunchKernelGGL(wrap_classify_kernel<DEST>, dim3(blocks_for(count)), dim3(256), 0, st, p->x, p->y, p->z, p->idcpu,
                       (long)first, (long)count, cg, lists, (long)capacity, dcount);
    WXA_LAUNCH_CHECK();
    if (!any_split) return WXA_OK;   // nothing can be listed: no need to wait
    unsigned h[NL];
    WXA_HIP_CHECK(hipMemcpyAsync(h, dcount, sizeof(h), hipMemcpyDeviceToHost, st));
    WXA_HIP_CHECK(hipStreamSynchronize(st));
    for (int c = 0; c < NL; ++c) counts[c] = h[c];
    return WXA_OK;
}

extern "C" {

wxa_status wxa_wrap_and_classify(const wxa_particle_view* p, int64_t first, int64_t count, const double prob_lo[3],
                                 const double prob_hi[3], const int periodic[3], const double brick_lo[3],
                                 const double brick_hi[3], const int split[3], int32_t* lists, int64_t capacity,
                                 int64_t counts[6], wxa_workspace* ws, void* stream) {
    return wrap_and_classify_impl<false>(p, first, count, prob_lo, prob_hi, periodic, brick_lo, brick_hi, split, lists,
                                         capacity, counts, ws, stream);
}

wxa_status wxa_wrap_and_classify_dest(const wxa_particle_view* p, int64_t first, int64_t count, const double prob_lo[3],
                                      const double prob_hi[3], const int periodic[3], const double brick_lo[3],
                                      const double brick_hi[3], const int split[3], int32_t* lists, int64_t capacity,
                                      int64_t counts[27], wxa_workspace* ws, void* stream) {
    return wrap_and_classify_impl<true>(p, first, count, prob_lo, prob_hi, periodic, brick_lo, brick_hi, split, lists,
                                        capacity, counts, ws, stream);
}

wxa_status wxa_pack_leavers(const wxa_particle_view* p, const int32_t* list, int64_t n, void* msg, int64_t row_len,
                            int64_t offset, int retire, const double brick_lo[3], const double brick_hi[3],
                            void* stream) {
    WXA_REQUIRE(pv_ok(p) && p->idcpu && brick_lo && brick_hi, "bad argument");
    WXA_REQUIRE(n >= 0 && (n == 0 || (list && msg)), "null list or message");
    WXA_REQUIRE(offset >= 0 && offset + n <= row_len, "list does not fit the message rows");
    if (n == 0) return WXA_OK;
    ClassifyGeom cg{};
    for (int d = 0; d < 3; ++d) { cg.blo[d] = brick_lo[d]; cg.bhi[d] = brick_hi[d]; }
    hipLaunchKernelGGL(pack_leavers_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, make_pv(*p),
                       list, (long)n, (double*)msg, (long)row_len, (long)offset, retire, cg);
    WXA_LAUNCH_CHECK();
    return WXA_OK;
}

wxa_status wxa_laser_push(const wxa_particle_view* p, const wxa_laser_push_params* c, double t, double dt,
                          void* stream) {
    WXA_REQUIRE(pv_ok(p) && c, "bad argument");
    WXA_REQUIRE(c->wavelength > 0 && c->waist > 0 && c->duration > 0, "laser: wavelength, waist and duration must be > 0");
    if (p->np == 0) return WXA_OK;
    using cplx = std::complex<double>;
    const cplx I(0, 1);
    const double k0 = 2. * M_PI / c->wavelength;
    const double inv_tau2 = 1. / (c->duration * c->duration);
    const double oscillation_phase = k0 * PhysConst::c * (t - c->t_peak);
    const cplx diffract_factor = 1. + I * c->focal_distance * 2. / (k0 * c->waist * c->waist);
    const cplx inv_complex_waist_2 = 1. / (c->waist * c->waist * diffract_factor);
    const cplx prefactor = c->e_max * std::exp(I * oscillation_phase) / diffract_factor;
    const cplx stcfactor = prefactor * std::exp(-cplx(inv_tau2 * (t - c->t_peak) * (t - c->t_peak), 0.0));
    LaserPushGeom lg;
    for (int d = 0; d < 3; ++d) { lg.position[d] = c->position[d]; lg.p_X[d] = c->p_X[d]; lg.p_Y[d] = c->p_Y[d]; }
    lg.mobility = c->mobility;
    lg.pre_re = stcfactor.real(); lg.pre_im = stcfactor.imag();
    lg.iw2_re = inv_complex_waist_2.real(); lg.iw2_im = inv_complex_waist_2.imag();
    lg.gamma_boost = c->gamma_boost > 1.0 ? c->gamma_boost : 1.0;
    const double beta_boost = lg.gamma_boost > 1.0 ? std::sqrt(1.0 - 1.0 / std::pow(lg.gamma_boost, 2.0)) : 0.0;
    for (int d = 0; d < 3; ++d) lg.drift[d] = lg.gamma_boost > 1.0 ? PhysConst::c * beta_boost * c->nvec[d] : 0.0;
    hipLaunchKernelGGL(laser_push_kernel, dim3(blocks_for(p->np)), dim3(256), 0, (hipStream_t)stream, make_pv(*p), lg, dt);
    WXA_LAUNCH_CHECK();
    return WXA_OK;
}

wxa_status wxa_apply_particle_boundaries(const wxa_particle_view* p, const double prob_lo[3],
                                         const double prob_hi[3], const int32_t bc_lo[3], const int32_t bc_hi[3],
                                         int64_t* n_lost, wxa_workspace* ws, void* stream) {
    WXA_REQUIRE(pv_ok(p) && prob_lo && prob_hi && bc_lo && bc_hi && ws, "bad argument");
    if (n_lost) *n_lost = 0;
    bool any = false;
    WallGeom wg;
    for (int d = 0; d < 3; ++d) {
        WXA_REQUIRE(prob_hi[d] > prob_lo[d], "empty domain");
        wg.lo[d] = prob_lo[d]; wg.hi[d] = prob_hi[d];
        wg.bc_lo[d] = bc_lo[d]; wg.bc_hi[d] = bc_hi[d];
        any = any || bc_lo[d] == WXA_PBOUNDARY_ABSORBING || bc_lo[d] == WXA_PBOUNDARY_REFLECTING ||
              bc_hi[d] == WXA_PBOUNDARY_ABSORBING || bc_hi[d] == WXA_PBOUNDARY_REFLECTING;
    }
    if (!any || p->np == 0) return WXA_OK;
    WXA_REQUIRE(p->idcpu, "idcpu is needed to retire absorbed particles");
    hipStream_t st = (hipStream_t)stream;
    wxa_status rc;
    if ((rc = ws->counters.reserve(COUNTER_BYTES)) != WXA_OK) return rc;
    unsigned* dcount = (unsigned*)ws->counters.p + CW_WALLS;
    WXA_HIP_CHECK(hipMemsetAsync(dcount, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(particle_walls_kernel, dim3(blocks_for(p->np)), dim3(256), 0, st, make_pv(*p), wg, dcount);
    WXA_LAUNCH_CHECK();
    if (n_lost) {
        unsigned h = 0;
        WXA_HIP_CHECK(hipMemcpyAsync(&h, dcount, sizeof(h), hipMemcpyDeviceToHost, st));
        WXA_HIP_CHECK(hipStreamSynchronize(st));
        *n_lost = h;
    }
    return WXA_OK;
}

// ---- the cell sort folded into PushPX (push_sort.hpp) ----------------------------------------------------------------
wxa_status wxa_push_sort_begin(wxa_workspace* ws, int32_t mode, const wxa_particle_view* p, const wxa_particle_view* dst,
                               const double plo[3], const double dinv[3], const int32_t cell_lo[3], const int32_t ncell[3],
                               const int32_t wrap[3], int32_t check_retired, double predict_dt, void* stream) {
    WXA_REQUIRE(ws && pv_ok(p), "bad argument");
    WXA_REQUIRE(mode == WXA_PUSH_SORT_COUNT || mode == WXA_PUSH_SORT_SCATTER || mode == (WXA_PUSH_SORT_COUNT | WXA_PUSH_SORT_SCATTER),
                "mode must be WXA_PUSH_SORT_COUNT, WXA_PUSH_SORT_SCATTER or both");
    auto& s = ws->ps;
    WXA_REQUIRE(s.armed == 0, "wxa_push_sort_begin without the wxa_push_sort_end of the previous one");
    WXA_REQUIRE(p->np < (1L << 31) - 2, "sizes exceed 32-bit sort keys");
    hipStream_t st = (hipStream_t)stream;
    const bool count = mode & WXA_PUSH_SORT_COUNT, scatter = mode & WXA_PUSH_SORT_SCATTER;
    // Everything that can fail comes first and what arms the pushes last: a begin that is refused leaves the workspace as
    // it found it.  One thing cannot wait: a lone COUNT writes into the buffers of the record nobody used, so that record
    // is dropped before they are touched, and stays dropped when an allocation or a memset then fails.
    if (scatter) {
        WXA_REQUIRE(s.pending.covers(p), "no record of a COUNT on these particle arrays (or they shrank since)");
        WXA_REQUIRE(pv_ok(dst) && dst->np >= p->np && (p->np == 0 || dst->x != p->x), "the destination tile: out of place, at least as long");
        WXA_REQUIRE((p->idcpu == nullptr) == (dst->idcpu == nullptr), "both tiles with ids or both without");
    }
    SortRecord armed;   // the tile being pushed and, for a COUNT, the cell box
    armed.x = p->x; armed.np = p->np;
    const int out = scatter ? 1 - s.in : s.in;   // a record nobody used is overwritten
    if (count) {
        WXA_REQUIRE(plo && dinv && cell_lo && ncell && wrap, "null argument");
        WXA_REQUIRE(ncell[0] > 0 && ncell[1] > 0 && ncell[2] > 0, "empty cell box");
        armed = SortRecord::of(p->x, p->np, plo, dinv, cell_lo, ncell);
        const long ncells = armed.bins;
        WXA_REQUIRE(ncells > 0 && ncells < (1L << 31) - 2, "sizes exceed 32-bit sort keys");
        if (!scatter) s.pending.valid = false;
        wxa_status rc;
        if ((rc = s.kr[out].reserve(sizeof(unsigned long long) * (size_t)(p->np + 1))) != WXA_OK) return rc;
        // the histogram and, behind it, the foreign counters; the own counts per cell
        if ((rc = s.hist.reserve(sizeof(int) * 2 * (ncells + 2))) != WXA_OK) return rc;
        if ((rc = s.offs[out].reserve(sizeof(int) * (ncells + 2))) != WXA_OK) return rc;
        if ((rc = s.own[out].reserve(sizeof(int) * (ncells + 2))) != WXA_OK) return rc;
        WXA_HIP_CHECK(hipMemsetAsync(s.hist.p, 0, sizeof(int) * 2 * (ncells + 2), st));
        WXA_HIP_CHECK(hipMemsetAsync(s.own[out].p, 0, sizeof(int) * (ncells + 2), st));
    }
    // nothing below fails
    if (count) {
        s.out = out;
        s.check_retired = check_retired && p->idcpu ? 1 : 0;
        s.predict_dt = predict_dt;
        for (int d = 0; d < 3; ++d) s.wrap[d] = wrap[d] ? 1 : 0;
    }
    if (scatter) {
        s.dst = *dst;
        s.appended = p->np - s.pending.np;
    }
    s.count = armed;
    s.armed = mode;
    return WXA_OK;
}

wxa_status wxa_push_sort_end(wxa_workspace* ws, int32_t read_live, int64_t* live, int64_t* appended, void* stream) {
    WXA_REQUIRE(ws && live && appended, "null argument");
    auto& s = ws->ps;
    WXA_REQUIRE(s.armed != 0, "wxa_push_sort_end without wxa_push_sort_begin");
    hipStream_t st = (hipStream_t)stream;
    const int32_t mode = s.armed;
    s.armed = 0;
    *live = s.count.np;
    *appended = 0;
    SortRecord next = s.count;   // what a COUNT leaves: its cell box, on the tile the pushes worked on ...
    if (mode & WXA_PUSH_SORT_SCATTER) {
        // the record's scan becomes the tile offsets of the LDS-tile kernels; the workspace now describes the destination tile
        ws->offsets.swap(s.offs[s.in]);
        int64_t n_live = s.pending.np;
        if (read_live) {   // retired particles were counted: the cell-sorted part ends where their bin starts
            int v = 0;
            WXA_HIP_CHECK(hipMemcpyAsync(&v, (const int*)ws->offsets.p + s.pending.bins, sizeof(int), hipMemcpyDeviceToHost, st));
            WXA_HIP_CHECK(hipStreamSynchronize(st));
            n_live = v;
        }
        ws->sorted = s.pending;
        ws->sorted.valid = true; ws->sorted.x = s.dst.x; ws->sorted.np = n_live;
        s.pending.valid = false;
        *live = n_live;
        *appended = s.appended;
        next.x = s.dst.x;   // ... or scattered them to
        next.np = n_live + s.appended;
    }
    if (mode & WXA_PUSH_SORT_COUNT) {
        const wxa_status rc = exclusive_scan((int*)s.hist.p, (int*)s.offs[s.out].p, (int)(next.bins + 2), ws, st);
        if (rc != WXA_OK) return rc;
        s.in = s.out;
        s.pending = next;
    }
    return WXA_OK;
}

int32_t wxa_push_sort_pending(const wxa_workspace* ws, const wxa_particle_view* p) {
    return ws && p && ws->ps.pending.covers(p) ? 1 : 0;
}

wxa_status wxa_sort_live_count(wxa_workspace* ws, int64_t* n, void* stream) {
    WXA_REQUIRE(ws && n, "null argument");
    WXA_REQUIRE(ws->sorted.valid, "no sort recorded in this workspace");
    int live = 0;
    hipStream_t st = (hipStream_t)stream;
    WXA_HIP_CHECK(hipMemcpyAsync(&live, (const int*)ws->offsets.p + ws->sorted.bins, sizeof(int), hipMemcpyDeviceToHost, st));
    WXA_HIP_CHECK(hipStreamSynchronize(st));
    ws->sorted.np = live;
    *n = live;
    return WXA_OK;
}

}  // extern "C"
