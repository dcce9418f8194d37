// Per-device scratch owned by the caller through wxa_workspace_create/destroy.
#ifndef WXA_WORKSPACE_HPP_
#define WXA_WORKSPACE_HPP_

#include "common.hpp"
#include "shapes.hpp"

#define WXA_TILE 8   // tile edge (cells) of the tile-major cell sort and of the LDS-tile kernels

namespace wxa {

// grow-only device buffer; owns its memory
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    void swap(DevBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); }
    wxa_status reserve(size_t bytes) {
        if (bytes <= cap) return WXA_OK;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 8 + 256;
        if (hipMalloc(&p, want) != hipSuccess) {
            set_last_error("hipMalloc of %zu bytes failed", want);
            return WXA_ERR_NOMEM;
        }
        cap = want;
        return WXA_OK;
    }
};

// Which cell sort a set of offsets describes: the particle array, how many of its particles they cover, the cell box.
// The workspace keeps three: the last sort, the record a COUNT left, and what is armed between begin and end.
struct SortRecord {
    bool valid = false;
    const double* x = nullptr;   // identity of the particle array
    int64_t np = 0;              // particles covered (of the last sort: the live ones after wxa_sort_live_count)
    int64_t bins = 0;            // cell bins (the retired bin follows)
    int32_t nc[3] = {0, 0, 0}, cell_lo[3] = {0, 0, 0};
    double plo[3] = {0, 0, 0}, dinv[3] = {0, 0, 0};   // physical lower corner of the cell box; cells are numbered from cell_lo

    // the first np particles of view p are the ones this record describes
    bool covers(const wxa_particle_view* p) const { return valid && x == p->x && np <= p->np; }
    static int tiles_of(int n) { return (n + WXA_TILE - 1) / WXA_TILE; }
    int tiles(int d) const { return tiles_of(nc[d]); }   // tiles per direction
    // cell bins of a box: whole tiles of WXA_TILE^3 cells
    static long bins_of(const int32_t nc[3]) {
        return (long)tiles_of(nc[0]) * tiles_of(nc[1]) * tiles_of(nc[2]) * (WXA_TILE * WXA_TILE * WXA_TILE);
    }
    static SortRecord of(const double* x, int64_t np, const double plo[3], const double dinv[3], const int32_t cell_lo[3],
                         const int32_t nc[3]) {
        SortRecord r;
        r.valid = true; r.x = x; r.np = np; r.bins = bins_of(nc);
        for (int d = 0; d < 3; ++d) { r.nc[d] = nc[d]; r.cell_lo[d] = cell_lo[d]; r.plo[d] = plo[d]; r.dinv[d] = dinv[d]; }
        return r;
    }
};

// ws->counters: COUNTER_BYTES of 32-bit words, the first word of each user
enum CounterWord : int {
    CW_DEPOSIT = 0,     // 0, 1: stragglers of the LDS-tile deposition, two slots (flip_counter)
    CW_GATHER = 16,     // 16, 17: stragglers of the LDS-tile gather, two slots
    CW_CLASSIFY = 32,   // 32 .. 37: the six lists of wxa_wrap_and_classify
    CW_WALLS = 48,      // particles lost to wxa_apply_particle_boundaries
    CW_INJECT = 56,     // 56, 57: particles added by wxa_add_plasma (64 bits)
    CW_DEST = 64,       // 64 .. 90: the 27 lists of wxa_wrap_and_classify_dest
    COUNTER_BYTES = 512
};

}  // namespace wxa

struct wxa_workspace {
    wxa::DevBuf cell, rank, hist, offsets, scan_tmp, stragglers, counters;
    wxa::DevBuf heavy;   // units per tile and the extra workgroups of the tiles that are split (heavy_tiles.hpp)
    // The straggler counts of the two LDS-tile kernels live in two slots each: launch n counts in slot n & 1, which launch
    // n - 1's tile kernel left at zero, and zeroes the other one for launch n + 1 -- no fill dispatch in front of the kernel
    // (round 6: a 4-byte hipMemsetAsync is a dispatch of 5 us; wxa::flip_counter below)
    bool flip_ready = false;
    unsigned gather_flips = 0, deposit_flips = 0;
    // the last cell sort: ws->offsets are its tile offsets (consumed by the LDS-tile kernels and the wrap through the sort)
    wxa::SortRecord sorted;
    // particles.E_external_particle / B_external_particle of the container that owns this workspace
    // (wxa_workspace_set_external_particle_fields); added to the gathered fields in PushPX / PushP
    double ext_eb[6] = {0, 0, 0, 0, 0, 0};
    // repeated plasma lens of that container (wxa_workspace_set_repeated_plasma_lens) and the time its fields are
    // evaluated at (wxa_workspace_set_time)
    wxa::DevBuf lens_tab, ext_pp;   // ext_pp: per-particle external fields of the current push (4 x np)
    int32_t lens_n = 0;
    double lens_period = 0, lens_dt = 0, lens_gamma_boost = 1, ext_time = 0;
    int64_t ext_pp_stride = 0;
    // accumulator type of the LDS-tile Esirkepov deposition (wxa_workspace_set_deposit_accumulator)
    int32_t deposit_accumulator = WXA_ACC_FP64;
    // the container's plasma streams through the grid (wxa_workspace_set_streaming_plasma): the LDS-tile Esirkepov
    // deposition takes every particle through the wide-frame body inside its loop (deposit_tile.hip, RowsCfg::WL)
    int32_t streaming_plasma = 0;
    // density and momentum expressions of the container's injector (wxa_workspace_set_injection_profile): the programs
    // in device memory, uploaded when they are set -- slot 0 the density, 1..3 the momenta; id 0 = none -- and the byte
    // per cell that the probe pass of wxa_add_plasma_profile leaves for its particle pass
    wxa::DevBuf inject_prog, inject_mask;
    uint64_t inject_id[4] = {0, 0, 0, 0};
    int32_t inject_off[4] = {0, 0, 0, 0}, inject_n[4] = {0, 0, 0, 0};
    // the cell sort folded into PushPX (push_sort.hpp; wxa_push_sort_begin / _end): what is armed for the pushes between
    // begin and end, and the record a COUNT left for the SCATTER of a later push
    struct PushSortState {
        int32_t armed = 0;                   // WXA_PUSH_SORT_* of the pushes between begin and end
        wxa::DevBuf kr[2], offs[2], own[2], hist;   // (key, rank) per particle, the scanned histogram and the own counts
                                                    // per cell, double-buffered; hist: the histogram and the foreign counters
        int32_t check_retired = 0;           // armed COUNT: the caller's tile may hold retired particles
        double predict_dt = 0.0;             // armed COUNT: keys of the positions this much free flight ahead
        int32_t in = 0, out = 0;             // kr[in], offs[in]: the pending record; [out]: what the armed COUNT writes
        wxa::SortRecord pending;             // the record kr[in], offs[in], own[in] hold, on the tile it indexes
        wxa::SortRecord count;               // armed: the tile being pushed (x, np) and, for a COUNT, the cell box it keys
        int32_t wrap[3] = {0, 0, 0};         // armed COUNT: the periodic directions
        wxa_particle_view dst{};             // armed SCATTER: the destination tile
        int64_t appended = 0;                // armed SCATTER: particles appended since the record was taken
    } ps;
};

namespace wxa {
// words `word`, `word + 1` of ws->counters as a two-slot counter (see wxa_workspace::flip_ready)
inline wxa_status flip_counter(wxa_workspace* ws, CounterWord word, unsigned& flips, hipStream_t st, unsigned*& cur, unsigned*& next) {
    wxa_status rc;
    if ((rc = ws->counters.reserve(COUNTER_BYTES)) != WXA_OK) return rc;
    if (!ws->flip_ready) {   // once per workspace
        WXA_HIP_CHECK(hipMemsetAsync(ws->counters.p, 0, COUNTER_BYTES, st));
        ws->flip_ready = true;
    }
    unsigned* base = (unsigned*)ws->counters.p + word;
    cur = base + (flips & 1u);
    next = base + ((flips + 1u) & 1u);
    ++flips;
    return WXA_OK;
}
// external fields of a push: the constants, and the per-particle ones once evaluate_particle_fields (particles.hip) has run
inline ExtEB ext_of(const wxa_workspace* ws) {
    ExtEB e{};
    if (!ws) return e;
    e.ex = ws->ext_eb[0]; e.ey = ws->ext_eb[1]; e.ez = ws->ext_eb[2];
    e.bx = ws->ext_eb[3]; e.by = ws->ext_eb[4]; e.bz = ws->ext_eb[5];
    if (ws->lens_n > 0 && ws->ext_pp_stride > 0) e.pp = ExtPerParticle{(const double*)ws->ext_pp.p, ws->ext_pp_stride};
    return e;
}
// the same for a view that starts `first` particles into the array the per-particle fields were evaluated on
inline ExtEB ext_of(const wxa_workspace* ws, int64_t first) {
    ExtEB e = ext_of(ws);
    if (e.pp.fields) e.pp.fields += first;
    return e;
}
inline ExtLens lens_of(const wxa_workspace* ws) {
    ExtLens L{};
    L.n = ws->lens_n;
    L.period = ws->lens_period;
    L.time = ws->ext_time;
    L.dt = ws->lens_dt;
    L.gamma_boost = ws->lens_gamma_boost;
    // m_uz_boost (GetExternalFields.cpp:28)
    L.uz_boost = std::sqrt(ws->lens_gamma_boost * ws->lens_gamma_boost - 1.0) * PhysConst::c;
    L.tab = (const double*)ws->lens_tab.p;
    return L;
}
// the LDS-tile kernels can take p: its first ws->sorted.np particles are those of the last cell sort
inline bool sorted_tiles_available(const wxa_workspace* ws, const wxa_particle_view* p) { return ws && ws->sorted.covers(p); }
// LDS-tile deposition (deposit_tile.hip)
wxa_status deposit_current_tiled(const wxa_particle_view* p, const wxa_field_view J[3],
                                 const wxa_grid_geom* geom, double q, double dt, double relative_time,
                                 int order, int algo, wxa_workspace* ws, hipStream_t stream);
// LDS-tile gather + push (gather_tile.hip); part: 0 every tile, or WXA_PART_INTERIOR / WXA_PART_REST of a PushPX
wxa_status gather_push_tiled(const wxa_particle_view* p, const wxa_field_view E[3], const wxa_field_view B[3],
                             const wxa_grid_geom* geom, double q, double m, double dt, int order, int galerkin,
                             int pusher, bool move, int part, wxa_workspace* ws, hipStream_t stream);
}  // namespace wxa
#endif
