// teal_gemv_plan.h — the launch plan of the 16-bit / int8 sparse GEMV: which kernel, which grid and which wave-local facts
// a request gets.  Pure host C++: integer arithmetic on shapes, a CU count and the values of a few pointers (their
// nullness, alignment and identities; none is dereferenced) — no HIP call, no global, no look at the workspace registry.
// run_gemv (teal_kernels.hip) plans and then launches what the plan says; teal_fused_gemv_plan answers from the same plan
// without a device.  The int4 GEMV keeps its own plan next to its kernel (teal_gemv_int4.hip: plan_i4); the producer checks the
// two share are check_producer below.
#pragma once
#include "teal_gemv_fast_decl.h"

#include <limits.h>
#include <stdio.h>

namespace teal {

// what teal_set_tuning / teal_set_wave_local / teal_set_fast / teal_set_phase_buffer hold in the diagnostics build (the
// product library passes constants): the caller reads them, the plan never does
struct GemvSwitches {
    Config force;    // 0 = not forced
    int wave_local;
    int fast;
    bool phase;      // a stamp buffer is set: 16-bit lean launches take the PHASE instantiation
};

enum GemvOutKind {
    kOutRounded,        // y rounded to dtype
    kOutRope,           // ... one q | k | v vector, RoPE and the KV-cache append in the epilogue (TEAL_OUT_QKV_ROPE)
    kOutPair,           // gate | up over the same column tile, y[0] = silu(gate) * up
    kOutSlabSum,        // one fp32 vector: the slices' sums folded in slice order (lean kernel only)
    kOutSlabs,          // fp32 slabs in an explicit destination, for a consumer that re-reads them in every workgroup
    kOutSlabsEpilogue,  // planar fp32 slabs in the caller's workspace, read once by an epilogue kernel
};

enum GemvFamily { kGemvLean, kGemvGeneral, kGemvGeneralReduce };  // (general + the ordered slab reduce launch)

// whose memory the partials go to
struct GemvMemory {
    void* ws;          // the caller's workspace: split-K partials of every kind but kOutSlabs
    size_t ws_bytes;
    bool ws_prepared;  // ... registered by teal_workspace_init: it starts with the arrival counters
    void* slabs;       // kOutSlabs: the destination
    size_t slabs_bytes;
    bool slabs_prepared;
};

struct GemvRequest {
    Params p;          // as the entry point filled it: producer, Z, the segments' w / y / tau / ld / col0 / ncols / scale, w8,
                       // act0, mask_out / mask_tau, the rope arguments.  pair, sum32, to_ws and the geometry are the plan's.
    int dtype;
    GemvOutKind kind;  // (kOutRope: where the lean kernel has the epilogue for this shape; else the request is served as kOutSlabs)
    bool interleave;   // kOutSlabs: slabs[col][slice]
    bool want_desc;
    GemvMemory mem;
};

// Where a request is served.  `launch` false: nowhere (teal_fused_gemv_plan) — it is planned for num_cu CUs, nothing is launched.
struct GemvSite {
    int num_cu;
    bool launch;
    hipStream_t st;
};
bool gemv_site(hipStream_t st, GemvSite& site);  // teal_kernels.hip: the current device (false: none)
// teal_fused_gemv over int4 group-quantised weights (out->weight_bits == 4): teal_gemv_int4.hip
int fused_gemv_i4(const teal_gemv_in_t* in, const teal_gemv_out_t* out, int Z, int dtype, const GemvMemory& mem, int* nslabs_out,
                  const GemvSite& site);

struct GemvPlan {
    int rc;
    Config c;
    GemvFamily family;
    Params p;          // complete but for the stamp buffer (p.phase: taken at launch)
    size_t lds;        // general kernel
    int krt;           // general kernel: the register-cache depth instantiated
    FastLaunch f;      // lean kernel (f.a.phase: taken at launch)
    bool rope;         // the rope epilogue is taken
    int nslabs;        // what the entry point reports in *nslabs_out
    char desc[160];    // the instantiation and grid as rocprofv3 prints them (want_desc)
};

constexpr size_t kListLdsBytes = 40 * 1024;  // LDS a workgroup's row lists may take: the launch stays inside the 64 KB a
                                             // workgroup gets without opting in to more

inline int vector_rounds(int Z) { return (((Z + 63) >> 6) + 15) / 16; }  // rounds of 16 chunks of 64 activations
inline int cache_depth(int rounds) { return rounds <= 4 ? 4 : (rounds <= 8 ? 8 : 16); }
inline bool list_fits(int Z, int split) { return (size_t)((Z + split - 1) / split) * 4 <= kListLdsBytes; }
inline int split_that_fits(int Z, int split) {
    while (!list_fits(Z, split) && split < kMaxSplit) ++split;
    return split;
}
// slices of the kept rows that bring `tiles` column tiles to about one workgroup per CU.  A slice of the wave-local
// compaction is a set of rounds, so no more slices than rounds; <= 8 keeps the slab count small for consumers that re-read them
inline int cover_split(int ncu, int tiles, int rounds) {
    int split = ncu / tiles;
    if (split > rounds) split = rounds;
    if (split > 8) split = 8;
    return split < 1 ? 1 : split;
}
inline bool class_70b(int Z, int ncols) { return (size_t)Z * ncols >= (size_t)8192 * 8192; }  // matrices from 8192 x 8192 up

// The geometry of a plain rounded 16-bit launch, before any adjustment for the output kind (teal_get_config reports it).
// Deterministic: no autotune at first call.  Measured on MI355X (profiles/, scripts/tune_gemv.py): the kernel wants ONE
// 16-wave workgroup per CU (every workgroup repeats the compaction prologue, so more workgroups only add latency), and
// a single launch (split == 1) whenever the column tiles alone can occupy >= ~60 % of the CUs.
inline Config default_geometry(int Z, int ncols_total, int ncu, const GemvSwitches& sw) {
    Config c = {0, 16, 1, 4};  // every instantiation is a 16-wave workgroup with unroll 4
    // widest tile whose tile count still covers most CUs -> no split-K, no second launch
    for (int lpr = 64; lpr >= 8; lpr >>= 1) {
        const int tiles = (ncols_total + lpr * 8 - 1) / (lpr * 8);
        if (tiles <= ncu + ncu / 8 && tiles * 5 >= ncu * 3) { c.lpr = lpr; break; }
    }
    if (c.lpr == 0) {
        const int t8 = (ncols_total + 63) / 64;
        if (t8 > ncu) {  // more 64-column tiles than CUs: widest tile that keeps >= ncu workgroups
            c.lpr = 8;
            for (int lpr = 64; lpr > 8; lpr >>= 1)
                if ((ncols_total + lpr * 8 - 1) / (lpr * 8) >= ncu) { c.lpr = lpr; break; }
        } else if (sw.wave_local && vector_rounds(Z) >= 2) {  // few columns: 64-column tiles, split the kept rows
            c.lpr = 8;
            c.split = cover_split(ncu, t8, vector_rounds(Z));
        } else {  // ... without the wave-local compaction, 512-byte row segments and a deeper split measured best
            c.lpr = ncols_total >= 2048 ? 32 : 8;
            const int tiles = (ncols_total + c.lpr * 8 - 1) / (c.lpr * 8);
            int split = ncu / tiles;
            const int max_by_rows = Z / (4 * c.waves * (64 / c.lpr));  // >= ~2 steps per workgroup at 50 %
            if (split > max_by_rows) split = max_by_rows;
            if (split < 1) split = 1;
            if (split > kMaxSplit) split = kMaxSplit;
            c.split = split;
        }
    }
    if (sw.force.lpr) c.lpr = sw.force.lpr;
    if (sw.force.split) c.split = sw.force.split;
    c.split = split_that_fits(Z, c.split);
    return c;
}

// The geometry of a launch: the default, adjusted once for the output kind and the weight width.  A forced tile width or
// split (diagnostics) switches the adjustments off.
inline Config choose_geometry(const Params& p, GemvOutKind kind, Config c, int total_cols, bool sliceable, int ncu,
                              const GemvSwitches& sw) {
    const bool forced = sw.force.split || sw.force.lpr;
    const int rounds = vector_rounds(p.Z);
    if (p.w8 && c.lpr > 32) c.lpr = 32;  // int8: 8 bytes per lane, tiles of at most 256 columns
    if (kind == kOutPair) {  // both matrices in one workgroup; the activation needs complete sums: no split-K
        c.split = 1;
        if (sw.force.lpr) return c;
        const int n1 = p.seg[0].ncols;
        c.lpr = 8;
        for (int lpr = 64; lpr > 8; lpr >>= 1)  // widest tile that still gives >= 2/3 of the CUs a tile
            if (((n1 + lpr * 8 - 1) / (lpr * 8)) * 3 >= ncu * 2) { c.lpr = lpr; break; }
        // a ragged second round (a 16-wave workgroup owns its CU): between one and 1.5 rounds of 64-column tiles — Llama-30B,
        // inter 17920 = 280 tiles on 256 CUs — run as ONE round of 128-column tiles when those cover at least half the CUs
        // (round 6, profiles/r06_ratio_vs_width.txt: 30B gate | up 56.2 us at 280 workgroups)
        const int t8 = (n1 + 63) / 64, t16 = (n1 + 127) / 128;
        if (c.lpr == 8 && t8 > ncu && t8 * 2 < ncu * 3 && t16 * 2 >= ncu) c.lpr = 16;
        return c;
    }
    if (forced) return c;
    const int t16 = (total_cols + 127) / 128;
    if (kind == kOutSlabs || kind == kOutSlabSum) {  // (a slab-sum launch is a slab launch whose last slice folds the slabs)
        const int wide = cover_split(ncu, t16, rounds);
        if (!p.w8 && class_70b(p.Z, total_cols) && t16 * wide * 10 >= ncu * 7 && list_fits(p.Z, wide)) {
            // slab output of a 70B-class matrix: 128-column tiles (256-byte row segments) with the kept rows sliced so that
            // tiles x slices ~ the CU count — fewer, longer row requests per CU.  Measured +2-8 % on those launches; on 7B / 8B
            // matrices the extra slices cost more in the consumers' prologues than they save (7B: 529 -> 518 tok/s), hence
            // the size gate.
            c.lpr = 16;
            c.split = wide;
        } else if (c.split > 1) {
            // the consumer re-reads every slab in each of its workgroups: prefer narrow tiles and a shallow split (64-column
            // tiles, <= 8 slabs) over 512-byte row segments.  No more slices than rounds, or the launch falls back to the
            // workgroup-wide list of the general kernel (round 5: the rank-local shapes of tensor parallelism — wo 2048 -> 4096
            // has two rounds, Llama-3-8B's wqkv / 2 four — ran 7.9-9.2 us that way, profiles/r05_tp_rank_local_launches.txt)
            const int tiles = (total_cols + 63) / 64;
            c.lpr = 8;
            c.split = split_that_fits(p.Z, cover_split(ncu, tiles, sw.wave_local ? rounds : 8));
            // a long vector can force more slices than CUs / tiles (LDS list capacity): then fill whole rounds of
            // workgroups (Llama-2-70B down, Z = 28672: 128 tiles x 3 slices = 1.5 rounds -> x 4 = 2 full rounds)
            while (tiles * c.split > ncu && (tiles * c.split) % ncu != 0 && c.split < 8) ++c.split;
        }
    }
    if (p.w8 && c.lpr < 16) {
        // int8: the stream is bound by cache-line REQUESTS per CU (measured: a 64-byte and a 128-byte row segment cost the
        // same, ~3.2 ns per row and CU), so a row segment should be a whole 128-byte line = 16 lanes = 128 columns, as long as
        // tiles x slices still cover half the CUs (half the CUs with 128-byte segments stream as much as all of them with
        // 64-byte segments, and 128-column tiles are what the lean kernel is built for: wo, 32 tiles x 4 slices).  The kept
        // rows may be sliced where the partials have somewhere to go: slab output, or arrival tickets.
        const int split = sliceable ? cover_split(ncu, t16, rounds) : 1;
        if (t16 * split * 2 >= ncu) {
            c.lpr = 16;
            c.split = split;
        }
    }
    return c;
}

// The wave-local compaction (no cross-wave list, no barriers before the stream): what one wave owns.  Derived once; the
// general launch takes wl / sl / krt / cap from here and the lean launch its cache depth and capacity — which is why the two
// kernels agree bit for bit on which slice sums which rows.
struct WaveLocal {
    bool ok;           // the lists fit and every slice owns a round
    bool slice_local;  // element-wise producers (everything but the RMSNorm, which needs the whole vector in every workgroup)
                       // cache only the rounds of the workgroup's slice
    int owned;         // rounds of the vector
    int need;          // rounds a workgroup caches
    int krt;           // register-cache depth
    int capw;          // list entries one wave can own
};
inline WaveLocal wave_local_facts(int Z, int mode, int split) {
    WaveLocal w;
    w.owned = vector_rounds(Z);
    w.slice_local = mode != 1 && split > 1;
    w.need = w.slice_local ? (w.owned + split - 1) / split : w.owned;
    w.krt = cache_depth(w.need);
    w.capw = (w.slice_local ? w.need : (w.krt + split - 1) / split) * 64;
    // (the merge producer's one lane per (cached chunk, split), krt * att_ns <= 64, holds for every Z teal_fused_gemv admits)
    w.ok = w.need <= w.krt && split <= w.owned && (size_t)16 * w.capw * 4 <= kListLdsBytes;
    return w;
}

inline size_t general_lds_bytes(int Z, int cap, int lpr, bool pair) {
    const int nch = (Z + 63) >> 6;
    return (size_t)nch * 8 + 128 + (size_t)cap * 4 + (size_t)16 * lpr * 8 * 4 * (pair ? 2 : 1) + 128;  // + int8 bias sums
}

// the lean kernel's per-wave list capacity (an element-wise producer lists only the rounds it caches) and its LDS
inline int lean_cap(const Params& p, const WaveLocal& w) { return p.in.mode == 1 ? w.capw : w.need * 64; }
inline size_t lean_lds_bytes(const Params& p, const Config& c, const WaveLocal& w) {
    return 64 + (size_t)16 * lean_cap(p, w) * 4 + (size_t)16 * c.lpr * 8 * 4 * (p.pair ? 2 : 1) + (p.w8 ? 128 : 0);
}

// Does this launch qualify for the lean kernel (teal_gemv_fast.h)?  Whole chunks and tiles, one weight image (or two:
// the gate|up pair, or gate | up as two unpaired segments), interleaved slabs or a single rounded output, wave-local
// lists that fit; 16-bit weights, or int8 images in 128-column tiles (never paired).
inline bool lean_shape(const Params& p, const Config& c, const WaveLocal& w, size_t ws_bytes, const GemvSwitches& sw) {
    if (!sw.fast || !p.wl || (c.lpr != 8 && c.lpr != 16)) return false;
    if (p.w8 && (c.lpr != 16 || p.pair)) return false;
    if ((p.Z & 63) || (p.in.mode != 1 && w.need > 8)) return false;
    const int bn = c.lpr * 8, mode = p.in.mode;
    // outputs: interleaved slabs for the next launch; one rounded vector (split == 1); or split > 1 folded into ONE
    // launch by arrival tickets (the last slice of a tile sums the partials in slice order)
    const bool ticketed = !p.to_ws && c.split > 1;
    if (c.split > 8 || (p.to_ws && !p.ws_il)) return false;
    if (ticketed && (!p.tickets || p.ntiles > kTicketTiles || !p.ws ||
                     ws_bytes < (size_t)((c.split + 3) & ~3) * (size_t)p.ws_ld * sizeof(float)))
        return false;
    const int nseg = p.pair ? 2 : p.nseg;
    int off = 0;
    for (int i = 0; i < nseg; ++i) {
        const Seg& sg = p.seg[i];
        if (sg.ncols % bn) return false;
        if (p.pair) continue;
        // one weight image cut into threshold segments (q|k|v) — or exactly two images, one per segment (gate | up unpaired)
        const bool same_image = sg.w == p.seg[0].w && sg.ld == p.seg[0].ld && sg.col0 == p.seg[0].col0 + off;
        if (!same_image && !(nseg == 2 && i == 1)) return false;
        if (p.w8 && same_image && reinterpret_cast<const uint16_t*>(sg.scale) != reinterpret_cast<const uint16_t*>(p.seg[0].scale) + off)
            return false;  // one image: its scale vector is one vector
        if (!p.to_ws && reinterpret_cast<const uint16_t*>(sg.y) != reinterpret_cast<const uint16_t*>(p.seg[0].y) + off) return false;
        off += sg.ncols;
    }
    if (p.pair && (mode != 1 || p.seg[0].ncols != p.seg[1].ncols)) return false;
    if (lean_lds_bytes(p, c, w) > 64 * 1024) return false;
    // mode 1 input: interleaved slabs, or ONE planar fp32 vector (the hand-over of a TEAL_OUT_SLAB_SUM launch)
    if (mode == 1 && ((p.in.nslabs > 0 && !p.in.slabs_il && p.in.nslabs != 1) || p.in.nslabs > 8)) return false;
    if (p.sum32 && (p.to_ws || p.pair || p.nseg != 1 || p.act0 || p.rope)) return false;
    if (p.rope &&  // RoPE + KV append epilogue: one rounded q|k|v vector, no split-K, tiles inside one head
        (mode != 1 || p.pair || p.w8 || p.to_ws || c.split != 1 || p.nseg != 3 || (p.rope_hd != 64 && p.rope_hd != 128) ||
         p.rope_hd % bn || p.seg[1].ncols != p.seg[2].ncols || p.seg[0].ncols % p.rope_hd || p.seg[1].ncols % p.rope_hd))
        return false;
    return true;
}

// the lean launch of a shape that qualifies, from the facts already in the plan
inline FastLaunch fill_fast(const Params& p, const Config& c, const WaveLocal& w) {
    const int mode = p.in.mode;
    const bool ticketed = !p.to_ws && c.split > 1;
    FastLaunch f = {};
    f.a.cap = lean_cap(p, w);
    f.lds = lean_lds_bytes(p, c, w);
    f.w8 = p.w8;
    f.mode = mode; f.pair = p.pair; f.lpr = c.lpr; f.ntiles = p.ntiles; f.split = c.split;
    f.kr = (mode != 1 && w.need <= 1) ? 1 : w.krt;
    f.Z = p.Z; f.nslabs = p.in.nslabs; f.eps = p.in.eps;
    switch (mode) {
        case 1: f.in0 = p.in.resid_in; f.in1 = p.in.slabs; f.in2 = p.in.norm_w; f.row_index = p.in.row_index;
                if (p.in.nslabs == 1 && !p.in.slabs_il) f.nslabs = 1 | 0x100;  // one planar vector: bit 8 of the count
                break;
        case 2: f.in0 = p.x; break;  // gate | up contiguous [2Z]
        case 3: f.in0 = p.x; f.in1 = p.in.masks; break;
        case 4: f.in0 = p.in.att; f.a.att_hd = p.in.att_hd; f.a.att_ns = p.in.att_ns;
                f.nslabs = p.in.att_ns | ((p.in.att_hd == 128 ? 7 : 6) << 8);  // the preloaded slot of the merge producer
                break;
        default: f.in0 = p.x; break;
    }
    const size_t wb = p.w8 ? 1 : 2;  // bytes per weight
    f.a.w0 = reinterpret_cast<const char*>(p.seg[0].w) + (size_t)p.seg[0].col0 * wb;
    f.a.ld0 = p.seg[0].ld;
    const bool two_images = !p.pair && p.nseg == 2 && !(p.seg[1].w == p.seg[0].w && p.seg[1].ld == p.seg[0].ld &&
                                                        p.seg[1].col0 == p.seg[0].col0 + p.seg[0].ncols);
    f.a.w1 = (p.pair || two_images) ? reinterpret_cast<const char*>(p.seg[1].w) + (size_t)p.seg[1].col0 * wb : nullptr;
    f.a.scale0 = reinterpret_cast<const uint16_t*>(p.seg[0].scale);
    f.a.scale1 = two_images ? reinterpret_cast<const uint16_t*>(p.seg[1].scale) : nullptr;
    f.a.ld1 = (p.pair || two_images) ? p.seg[1].ld : 0;
    f.a.w1_tile = two_images ? p.seg[1].tile0 : INT_MAX;
    f.a.y = p.seg[0].y;
    f.a.ws = p.ws;
    f.a.mask_out = p.mask_out;
    f.a.mask_tau = p.mask_tau;
    f.a.resid_out = p.in.resid_out;
    f.a.tau0 = p.seg[0].tau; f.a.tau1 = p.seg[1].tau; f.a.tau2 = p.seg[2].tau;
    f.a.seg_tile1 = (!p.pair && p.nseg > 1) ? p.seg[1].tile0 : INT_MAX;
    f.a.seg_tile2 = (!p.pair && p.nseg > 2) ? p.seg[2].tile0 : INT_MAX;
    f.a.act0 = p.act0;
    f.a.sum32 = p.sum32;
    f.a.gate_act = p.in.gate_act;
    f.a.ws_stride = (p.to_ws || ticketed) ? ((c.split + 3) & ~3) : 0;
    f.a.ticket = ticketed ? p.tickets : nullptr;
    if (p.rope) {
        f.a.rope = p.rope; f.a.rope_pos = p.rope_pos; f.a.kc = p.kc; f.a.vc = p.vc;
        f.a.rope_hd = p.rope_hd; f.a.rope_dim = p.seg[0].ncols; f.a.rope_kv = p.seg[1].ncols; f.a.rope_max_seq = p.rope_max_seq;
    }
    return f;
}

// One launch of one output kind: validation, geometry, wave-local facts, workspace, kernel family, description.
// kOutRope where the shape is not the lean kernel's: the request is planned again as kOutSlabs.
inline int plan_kind(const GemvRequest& r, GemvOutKind kind, const Config& dflt, int total_cols, int ncu,
                     const GemvSwitches& sw, GemvPlan& out) {
    const bool rope = kind == kOutRope;
    Params& p = out.p;
    p = r.p;
    p.pair = kind == kOutPair ? 1 : 0;
    p.sum32 = kind == kOutSlabSum ? 1 : 0;
    p.to_ws = (kind == kOutSlabs || kind == kOutSlabsEpilogue) ? 1 : 0;
    if (rope) {  // (k, v land in the caches; the lean kernel wants one vector)
        p.seg[1].y = reinterpret_cast<uint16_t*>(p.seg[0].y) + p.seg[0].ncols;
        p.seg[2].y = reinterpret_cast<uint16_t*>(p.seg[0].y) + p.seg[0].ncols + p.seg[1].ncols;
    } else {
        p.rope = nullptr; p.rope_pos = nullptr; p.kc = nullptr; p.vc = nullptr;
        p.rope_hd = 0; p.rope_max_seq = 0;
    }
    // where the partials go: the explicit destination, or the caller's workspace — behind the header that holds the arrival
    // counters when it is a prepared one
    void* ws = r.mem.ws;
    size_t ws_bytes = r.mem.ws_bytes;
    p.tickets = nullptr;
    if (kind == kOutSlabs) {
        if (!r.mem.slabs || r.mem.slabs_prepared) return TEAL_ERR_ARG;  // a prepared workspace starts with the library's header
        ws = r.mem.slabs;
        ws_bytes = r.mem.slabs_bytes;
    } else if (r.mem.ws_prepared) {
        p.tickets = ws_tickets(ws);
        ws = ws_slabs(ws);
        ws_bytes -= kWsHeaderBytes;
    }
    if (p.w8)
        for (int i = 0; i < (p.pair ? 2 : p.nseg); ++i)
            if (!p.seg[i].scale || (p.seg[i].ld & 7) || (p.seg[i].col0 & 7)) return TEAL_ERR_ARG;
    if ((p.in.mode == 1 || p.in.mode == 4) && p.Z > 16 * 64 * 16) return TEAL_ERR_SHAPE;  // register-resident producer
    if (p.pair && (size_t)(p.Z + 1) * 4 > 44 * 1024) return TEAL_ERR_SHAPE;

    const Config c = choose_geometry(p, kind, dflt, total_cols, p.to_ws || p.tickets, ncu, sw);
    out.c = c;
    const int bn = c.lpr * 8;
    int t = 0, off = 0;
    for (int i = 0; i < (p.pair ? 1 : p.nseg); ++i) {
        p.seg[i].tile0 = t;
        p.seg[i].ws_off = off;
        t += (p.seg[i].ncols + bn - 1) / bn;
        off += p.seg[i].ncols;
    }
    if (p.pair) p.nseg = 1;  // tile space = the gate columns; seg[1] rides along
    p.ntiles = t;
    p.split = c.split;
    p.ws_ld = off;
    const WaveLocal w = wave_local_facts(p.Z, p.in.mode, c.split);
    p.wl = (sw.wave_local && w.ok) ? 1 : 0;
    p.sl = (p.wl && w.slice_local) ? 1 : 0;
    p.krt = p.wl ? w.krt : 0;
    p.cap = p.wl ? w.capw : (p.Z + c.split - 1) / c.split + 1;
    p.ws = reinterpret_cast<float*>(ws);
    out.krt = cache_depth(p.wl ? w.krt : w.owned);
    out.lds = general_lds_bytes(p.Z, p.wl ? p.cap * 16 : p.cap, c.lpr, p.pair != 0);
    if (out.lds > 64 * 1024) return TEAL_ERR_SHAPE;
    p.ws_il = (r.interleave && kind == kOutSlabs && c.split <= 8) ? 1 : 0;
    if (c.split > 1 || p.to_ws) {
        const size_t slabs = p.ws_il ? (size_t)((c.split + 3) & ~3) : (size_t)c.split;
        if (!ws || ws_bytes < slabs * off * sizeof(float)) return TEAL_ERR_WORKSPACE;
        if (!aligned16(ws)) return TEAL_ERR_ALIGN;
    }
    out.nslabs = kind == kOutSlabSum ? 1 : c.split;
    out.rope = false;
    if (lean_shape(p, c, w, ws_bytes, sw)) {
        const FastLaunch& f = out.f = fill_fast(p, c, w);
        out.family = kGemvLean;
        out.rope = rope;
        if (rope) out.nslabs = 0;
        // (the instantiation as rocprofv3 prints it: BF16, MODE, PAIR, LPR, KR, EXACT, PHASE, U, W8, ROPE)
        if (r.want_desc)
            snprintf(out.desc, sizeof out.desc, "gemv_fast_kernel<%s,%d,%s,%d,%d,%s,%s%s,%s> grid (%d,%d) x 1024",
                     r.dtype == TEAL_BF16 ? "true" : "false", f.mode, f.pair ? "true" : "false", f.lpr, f.kr,
                     (f.mode == 1 && f.Z == 1024 * f.kr) ? "true" : "false", (sw.phase && !f.w8) ? "true" : "false",
                     f.w8 ? ",4,true" : ",4,false", f.a.rope ? "true" : "false", f.ntiles, f.split);
        return TEAL_OK;
    }
    // the RoPE epilogue and the fp32 slice sum exist in the lean kernel only
    if (rope) return plan_kind(r, kOutSlabs, dflt, total_cols, ncu, sw, out);
    if (p.sum32) return TEAL_ERR_CONFIG;
    out.family = (c.split > 1 && !p.to_ws) ? kGemvGeneralReduce : kGemvGeneral;
    if (r.want_desc)
        snprintf(out.desc, sizeof out.desc, "sparse_gemv_kernel<%d,%d,%d,%s,%d,%d,%s,%s> grid %d x %d", c.lpr, c.waves, c.unroll,
                 r.dtype == TEAL_BF16 ? "true" : "false", p.in.mode, out.krt, p.pair ? "true" : "false", p.w8 ? "true" : "false",
                 p.ntiles * p.split, c.waves * 64);
    if (r.interleave && kind == kOutSlabs && !p.ws_il) return TEAL_ERR_CONFIG;  // > 8 slices cannot interleave
    return TEAL_OK;
}

// The plan of a request on a device with `num_cu` CUs.  Returns (and leaves in out.rc) what the launch returns.
inline int plan_gemv(const GemvRequest& r, int num_cu, const GemvSwitches& sw, GemvPlan& out) {
    out.desc[0] = 0;
    out.nslabs = 0;
    int total_cols = 0;
    for (int i = 0; i < r.p.nseg; ++i) total_cols += r.p.seg[i].ncols;
    const Config dflt = default_geometry(r.p.Z, total_cols, num_cu, sw);
    GemvOutKind kind = r.kind;
    // the fused epilogue exists in the lean kernel for a launch without split-K; a 70B-class projection hands over
    // row-sliced slabs of 128-column tiles instead (measured faster there, profiles/r04_layer_experiments.txt)
    if (kind == kOutRope && !(dflt.split == 1 && !class_70b(r.p.Z, total_cols) && sw.fast && !sw.force.split && !sw.force.lpr))
        kind = kOutSlabs;
    return out.rc = plan_kind(r, kind, dflt, total_cols, num_cu, sw, out);
}

// What teal_fused_gemv asks of its producer whatever the weight width; kProducerInt4: the int4 kernel's narrower rules
// (interleaved input slabs only, the whole vector in 32 KB of LDS for the RMSNorm, no MASKED form; it has no merge-lane limit).
enum ProducerRules { kProducer16or8, kProducerInt4 };
inline int check_producer(const teal_gemv_in_t* in, int Z, ProducerRules rules) {
    const bool int4 = rules == kProducerInt4;
    switch (in->mode) {
        case TEAL_IN_PLAIN:
        case TEAL_IN_SILU_MUL:
            return in->x ? TEAL_OK : TEAL_ERR_ARG;
        case TEAL_IN_ATTN_MERGE:
            if (!in->x || (in->att_head_dim != 64 && in->att_head_dim != 128) || Z % in->att_head_dim ||
                (in->att_nsplit != 0 && in->att_nsplit != 4 && in->att_nsplit != 8))
                return TEAL_ERR_ARG;
            if (!int4 && Z > (64 / (in->att_nsplit ? in->att_nsplit : 4)) * 1024) return TEAL_ERR_SHAPE;  // one lane per (chunk, split)
            return TEAL_OK;
        case TEAL_IN_MASKED:
            return (int4 || !in->x || !in->masks) ? TEAL_ERR_ARG : TEAL_OK;
        case TEAL_IN_RESID_NORM:
            if (!in->resid_in || !in->norm_weight || in->nslabs < 0 || (in->nslabs > 0 && !in->slabs)) return TEAL_ERR_ARG;
            if (in->resid_out == in->resid_in && !in->row_index) return TEAL_ERR_ARG;  // must ping-pong
            if (int4 ? (in->nslabs > 0 && (!in->slabs_interleaved || in->nslabs > 8 || !aligned16(in->slabs)))
                     : (in->slabs_interleaved && in->nslabs > 8))
                return TEAL_ERR_ARG;
            if (int4 && Z > 16384) return TEAL_ERR_SHAPE;  // 16 elements per thread, 32 KB of LDS
            return TEAL_OK;
        default: return TEAL_ERR_ARG;
    }
}

}  // namespace teal
