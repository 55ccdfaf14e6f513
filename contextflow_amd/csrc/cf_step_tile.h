// The forward step on 32x32x2 tiles, SPW whole samples per workgroup: flow_step_phases, k_flow_step, its level form
// k_flow_step_level and their launch helpers.  Included by cf_step.hip, which holds the launch lists that instantiate them;
// everything lives in an anonymous namespace of the including translation unit.
#pragma once
#include "cf_step_fwd.h"
#include <atomic>

namespace {

// ---- the step kernel ---------------------------------------------------------------------------------
// One workgroup per tile of SPW samples.  Per wave (all wave-local unless noted; a wave owns the pixel
// columns of its PTW tiles):
//   x (16-byte loads) -> registers -> LDS plane Xp[ch][pix]
//   phase 0  y = W'x + b'        (MFMA, B operand from Xp)   -> y0 -> LDS Y0, y1 stays in registers
//            z[:, :C/2] = y0     written from Y0 with 16-byte stores
//   phase 1  h1 = relu(NN.0 y0)  -> LDS H1 ;  BARRIER (3x3 taps read neighbouring waves' columns)
//   phase 2  3x3 reflect conv    ;  BARRIER (everyone done reading h1) ;  h2 -> LDS (in place)
//   phase 3  h = NN.4 h2 ; affine map ; z[:, C/2:] via LDS with 16-byte stores ; per-sample log-det
// SQ: x is the UN-squeezed tensor (B, C/4, 2H, 2W); Squeeze((2,2)) (squeeze.py:10-11) is folded into the x
// staging: one 16-byte load along the un-squeezed row = channels (4c'+2i1, +1) of squeezed pixels (x, x+1).
// dbg (optional, tests only): dumps of y0, h1, h2, h as [rows][tiles*PIX].
// CTX: per-sample bias of the specialist coupling (see conditioner_net); sb = (B, C) or (B, 2C) floats.
// DUMP (training): y0 and the post-ReLU h1 / h2 planes are also written to the tape `tp`; the backward kernel then
// loads them instead of recomputing phases 1 and 2 (cf_step_bwd.h, TAPED).
// DBG: the test-only instantiation that honours `dbg`; the production kernels carry no dump branches at all.
// Phases 0-3, the affine map and the log-det of ONE step on the x plane that sits in rows [0, C) of H1 (this wave's own columns):
// the one body of the single-step kernel and of the level kernel below.
// LEVEL: the step is one of a run that stays in LDS (k_flow_step_level).  Nothing of z goes to global memory here; at the end z =
// [y0 | z1] is the NEXT step's x plane - y0 moves from the Y0 plane (every lane takes back the words it wrote itself), z1 goes
// straight from the registers.  Cross-wave hazards of that hand-off: none that the step's own barriers do not cover.  The plane
// rows are this wave's own columns, which no other wave reads (phase 0) and which the NEXT step overwrites with h1 only behind
// the workgroup barrier in front of those writes (conditioner_net: the skewed / parity-split h1 order) - a barrier that every
// wave reaches only after its own phase 3 of THIS step; the log-det finishes inside the wave (HW <= 32 PTW).
template <class G, int CTX, bool DUMP, bool DBG, bool LEVEL>
__device__ __forceinline__ void flow_step_phases(float* __restrict__ z, float* __restrict__ ldj_acc, const float* __restrict__ wsl, int B,
                                                 float* __restrict__ dbg_arg, const float* __restrict__ sb, StepTape tp, int tile, int wave_u = 0) {
    float* const dbg = DBG ? dbg_arg : nullptr;
    constexpr int C = G::C, HW = G::HW, PIX = G::PIX, HALF = G::HALF, HID = G::HID;
    constexpr int PTW = G::PTW, RT03 = G::RT03;
    constexpr int WPX = 32 * PTW;                     // pixel columns owned by one wave
    static_assert(!LEVEL || (CTX == 0 && !DUMP && !DBG && HW <= 32 * PTW), "level form: the evaluation step, log-det inside the wave");
    extern __shared__ __align__(16) float lds[];      // G::LDS_FLOATS floats (up to 160 KiB: dynamic)
    float* Y0 = lds;                    // [HALF][PIX]   y0 (phase 0 -> 1), later the z1 staging plane
    float* H1 = lds + HALF * PIX;       // [HID][PIX]    x plane (rows < C), then h1, then h2 in place

    // FRESH: the lane's indices are formed again behind the 3x3, from the wave's index in a scalar register, instead of living
    // across it.  The zero-skipping geometry needs that as the level form does: carried, they cost it 15 spilled registers
    constexpr bool FRESH = LEVEL || G::ZSKIP;
    static_assert(!G::ZSKIP || (CTX == 0 && !DUMP && !DBG), "zero skip: the evaluation step");
    const int tid_ = FRESH ? wave_u * 64 + cf_lane_fresh() : (int)threadIdx.x;      // (LEVEL: per step, see cf_lane_fresh)
    const int tid = tid_, wave = tid >> 6;
    int lane = tid & 63, li = lane & 31, lk = lane >> 5;
    const int ntiles = (B + G::SPW - 1) / G::SPW;
    const int64_t dbg_cols = (int64_t)ntiles * PIX;

    int pix[PTW], pin[PTW];             // this lane's pixel column inside the workgroup / inside its sample
#pragma unroll
    for (int q = 0; q < PTW; ++q) {
        pix[q] = (wave * PTW + q) * 32 + li;
        pin[q] = pix[q] % HW;
    }
    {
        const int b0 = tile * G::SPW;
        int smp[PTW];
        bool live[PTW];
#pragma unroll
        for (int q = 0; q < PTW; ++q) { smp[q] = b0 + pix[q] / HW; live[q] = smp[q] < B; }

        cf_wave_sync();                 // x plane: written 16 bytes per lane, read as MFMA operands by other lanes

        // ================= phase 0: y = (e^{-logs} Wm) x - t e^{-logs}        (conv1x1.py:54 + actnorm.py:59)
        f32x16 acc0[RT03][PTW];
#pragma unroll
        for (int rt = 0; rt < RT03; ++rt)
#pragma unroll
            for (int q = 0; q < PTW; ++q) acc0[rt][q] = bias_tile(wsl + G::OFF_B0 + rt * 32, lk);
        dense_phase<G, G::KS0, G::NG0, RT03>(acc0, ws_rsrc(wsl, G::WS_FLOATS), G::OFF_A0, H1, pix, lane);
        // first half: conditioner input -> LDS, and it is also the first half of the output (coupling.py:65);
        // second half (x1 after Conv1x1+ActNorm) stays in registers until the epilogue
        float y1[PTW][HALF <= 16 ? 8 : 16];
#pragma unroll
        for (int q = 0; q < PTW; ++q)
#pragma unroll
            for (int r = 0; r < (HALF <= 16 ? 8 : 16); ++r) {
                const int idx = tile_row(r, lk);                 // channel index inside its half
                if (idx < HALF) Y0[idx * PIX + pix[q]] = acc0[0][q][r];
                y1[q][r] = (HALF <= 16) ? acc0[0][q][r + 8] : acc0[RT03 - 1][q][r];
            }
        if constexpr (LEVEL) {
            // y1 is pinned HERE: inside the level loop hipcc otherwise sinks the MFMAs of the y1 row tile behind phase 2, next to
            // their first use, and carries their operands - fragments and x values - there through scratch (50 registers at C = 64)
#pragma unroll
            for (int q = 0; q < PTW; ++q)
#pragma unroll
                for (int r = 0; r < (HALF <= 16 ? 8 : 16); ++r) asm volatile("" : "+v"(y1[q][r]));
        }
        cf_wave_sync();                 // y0 plane complete for this wave's columns
        if constexpr (!LEVEL) z_store<G>(z, Y0, b0, 0, B, wave, lane);
        if constexpr (DUMP) rows_store_t<G, HALF, HALF>(tp.y0, Y0, b0, B, wave, lane);
        if (dbg) {
            __syncthreads();
            for (int e = tid; e < HALF * PIX; e += G::NT) dbg[(int64_t)(e / PIX) * dbg_cols + (int64_t)tile * PIX + (e % PIX)] = Y0[e];
            __syncthreads();
        }

        f32x16 acc3[RT03][PTW];
        if constexpr (FRESH) {
            // phases 1 and 2, then the lane's indices AGAIN and phase 3 with those: nothing but y1 is live across the 3x3, which fills
            // the register file (the 8x8 kernel sits at 256 registers; carried, the indices cost the level form 4 spilled ones)
            conditioner_net<G, 0, false, 2>(acc3, lds, wsl, pix, pin, lane, tid, nullptr, 0, tile, nullptr, nullptr, tp, B);
            lane = cf_lane_fresh(); li = lane & 31; lk = lane >> 5;
            if constexpr (G::ZSKIP) lk &= 1;      // (says lk < 2: the `idx < HALF` tests of the epilogue below then fold away)
#pragma unroll
            for (int q = 0; q < PTW; ++q) {
                pix[q] = (wave_u * PTW + q) * 32 + li;
                pin[q] = pix[q] % HW;
                smp[q] = b0 + pix[q] / HW;
                live[q] = smp[q] < B;
            }
#pragma unroll
            for (int rt = 0; rt < RT03; ++rt)
#pragma unroll
                for (int q = 0; q < PTW; ++q) acc3[rt][q] = bias_tile(wsl + G::OFF_B3 + rt * 32, lk);
            dense_phase<G, G::KS3, G::NG3, RT03>(acc3, ws_rsrc(wsl, G::WS_FLOATS), G::OFF_A3, H1, pix, lane);
        } else if constexpr (CTX == 0) {
            conditioner_net<G, 0, DUMP>(acc3, lds, wsl, pix, pin, lane, tid, dbg, dbg_cols, tile, nullptr, nullptr, tp, B);
        } else {
            int soff[PTW];
#pragma unroll
            for (int q = 0; q < PTW; ++q) soff[q] = min(smp[q], B - 1) * (CTX == 1 ? C : HID);
            conditioner_net<G, CTX, DUMP>(acc3, lds, wsl, pix, pin, lane, tid, dbg, dbg_cols, tile, sb, soff, tp, B);
        }
        if constexpr (LEVEL) cf_wave_sync();      // phase 3 has read h2 (other lanes' rows of these columns): rows < C are free

        float lsum[PTW];
#pragma unroll
        for (int q = 0; q < PTW; ++q) {
            lsum[q] = 0.f;
#pragma unroll
            for (int r = 0; r < (HALF <= 16 ? 8 : 16); ++r) {
                const int idx = tile_row(r, lk);
                if (idx < HALF) {
                    const float tt = acc3[0][q][r];
                    const float raw = (HALF <= 16) ? acc3[0][q][r + 8] : acc3[RT03 - 1][q][r];
                    const float ls = cf_log_scale(raw);
                    if constexpr (LEVEL) {          // [y0 | z1] = the next step's x plane (or the plane the level's epilogue stores)
                        H1[(HALF + idx) * PIX + pix[q]] = fmaf(y1[q][r], __expf(ls), tt);
                        H1[idx * PIX + pix[q]] = Y0[idx * PIX + pix[q]];
                    } else {
                        Y0[idx * PIX + pix[q]] = fmaf(y1[q][r], __expf(ls), tt);      // coupling.py:63 (z1, staged in LDS)
                    }
                    lsum[q] += ls;
                    if constexpr (DUMP) {           // tape: 128 contiguous bytes per row and half wave
                        if (live[q]) {
                            const int64_t o = ((int64_t)smp[q] * HALF + idx) * HW + pin[q];
                            tp.ls[o] = ls;
                            tp.y1[o] = y1[q][r];
                        }
                    }
                    if (dbg) {
                        float* d = dbg + (int64_t)(C + 2 * HID) * dbg_cols + (int64_t)tile * PIX + pix[q];
                        d[(int64_t)idx * dbg_cols] = tt;
                        d[(int64_t)(HALF + idx) * dbg_cols] = raw;
                    }
                }
            }
        }
        cf_wave_sync();                 // z1 plane complete for this wave's columns
        if constexpr (!LEVEL) {
            z_store<G>(z, Y0, b0, HALF, B, wave, lane);
            cf_wave_sync();             // ... and read back, before the log-det scratch below reuses those words
        }

        // per-sample reduction of log_s: lanes of one sample inside a 32-pixel tile first (shuffles) ...
        constexpr int SEG = HW < 32 ? HW : 32;            // lanes (pixels) of one sample inside a tile
        float v[PTW];
#pragma unroll
        for (int q = 0; q < PTW; ++q) {
            v[q] = lsum[q];
#pragma unroll
            for (int o = 1; o < SEG; o <<= 1) v[q] += __shfl_xor(v[q], o, 64);
            v[q] += __shfl_xor(v[q], 32, 64);
        }
        if constexpr (HW <= 32 * PTW) {
            // ... whole samples live inside this wave: finish in registers, the first lane of a sample owns ldj_acc[b]
            // (LEVEL: the same lane adds the per-step terms of its sample one step after the other - the order of n launches)
            constexpr int TPS = HW >= 32 ? HW / 32 : 1;   // tiles per sample
#pragma unroll
            for (int q = 0; q < PTW; q += TPS) {
                float sum = v[q];
#pragma unroll
                for (int i = 1; i < TPS; ++i) sum += v[q + i];
                if (lk == 0 && (li % SEG) == 0 && live[q]) ldj_acc[smp[q]] += wsl[0] + sum;
            }
        } else {
            // ... a sample spans several waves: one LDS hop through this wave's own columns of Y0 (its z1 values have
            // been read back already); the second barrier keeps the next tile's y0 from overwriting the scratch
            constexpr int TPS = HW / 32;
#pragma unroll
            for (int q = 0; q < PTW; ++q)
                if (lane == 0) Y0[wave * WPX + q] = v[q];
            __syncthreads();
            if (tid < G::SPW && b0 + tid < B) {
                float sum = 0.f;
#pragma unroll
                for (int i = 0; i < TPS; ++i) {
                    const int t = tid * TPS + i;                       // tile index inside the workgroup
                    sum += Y0[(t / PTW) * WPX + (t % PTW)];
                }
                ldj_acc[b0 + tid] += wsl[0] + sum;
            }
            __syncthreads();
        }
    }
}

template <class G, bool SQ, int CTX = 0, bool DUMP = false, bool DBG = false>
__global__ __launch_bounds__(G::NT, G::MINW) void k_flow_step(const float* __restrict__ x, float* __restrict__ z,
                                                   float* __restrict__ ldj_acc, const float* __restrict__ ws, int B,
                                                   int64_t xbs, float* __restrict__ dbg_arg, int flags,
                                                   const float* __restrict__ sb, StepTape tp) {
    constexpr int XI = G::C * G::PTW / 8;             // 16-byte x items per lane and tile
    extern __shared__ __align__(16) float lds[];
    float* H1 = lds + G::HALF * G::PIX;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    (void)flags;

    // One tile per workgroup (grid = ntiles).  A persistent tile loop with the next tile's x prefetched into
    // registers was tried: hipcc then keeps 50-110 more VGPRs live across the loop (occupancy 4 -> 2 at C=16) and
    // it measured slower; co-resident workgroups hide the x-load latency instead.
    float4 xr[XI];
    const int tile = blockIdx.x;
    x_load<G, SQ>(xr, x, xbs, tile, B, wave, lane);
    x_to_lds<G, SQ>(xr, H1, wave, lane);
    if constexpr (G::ZSKIP) flow_step_phases<G, CTX, DUMP, DBG, false>(z, ldj_acc, ws, B, dbg_arg, sb, tp, tile, __builtin_amdgcn_readfirstlane(wave));
    else flow_step_phases<G, CTX, DUMP, DBG, false>(z, ldj_acc, ws, B, dbg_arg, sb, tp, tile);
}
// Level form (cf_flow_step_fwd_level): the n <= kChain steps of one resolution level on this workgroup's samples in ONE launch, z in
// LDS from step to step.  x is fetched once (squeeze-folded where the level begins behind a Squeeze), the loop has one body for
// every step and carries the step index alone, and z goes out once behind it, from the plane, as whole channel rows.
template <class G, bool SQ>
__global__ __launch_bounds__(256, G::MINW) void k_flow_step_level(const float* __restrict__ x, float* __restrict__ z,
                                                                  float* __restrict__ ldj_acc, const WsChain wc, int nsteps, int B, int64_t xbs) {
    constexpr int XI = G::C * G::PTW / 8;
    extern __shared__ __align__(16) float lds[];
    float* H1 = lds + G::HALF * G::PIX;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x, wave_u = __builtin_amdgcn_readfirstlane(wave);
    {
        float4 xr[XI];
        x_load<G, SQ>(xr, x, xbs, tile, B, wave, lane);
        x_to_lds<G, SQ>(xr, H1, wave, lane);
    }
#pragma unroll 1
    for (int st = 0; st < nsteps; ++st) flow_step_phases<G, 0, false, false, true>(z, ldj_acc, wc.ws[st], B, nullptr, nullptr, kNoTape, tile, wave_u);
    rows_store<G, G::C>(z, H1, tile * G::SPW, 0, B, wave_u, cf_lane_fresh());       // (its addresses are formed here, not beside x_load's)
}

template <class G, bool SQ, int CTX, bool DUMP, bool DBG>
int launch_step_sq(const StepArgs& a) {
    constexpr size_t lds_bytes = (size_t)G::LDS_FLOATS * sizeof(float);
    if (lds_bytes > 64 * 1024) {          // one-time opt-in to > 64 KiB of dynamic LDS (immutable afterwards)
        static std::atomic<uint64_t> raised{0};
        if (int rc_ = cf_raise_dynamic_lds((const void*)k_flow_step<G, SQ, CTX, DUMP, DBG>, 160 * 1024, raised, __func__)) return rc_;
    }
    const int grid = (a.B + G::SPW - 1) / G::SPW;
    // (the kernel's `flags` argument is unused: 0)
    k_flow_step<G, SQ, CTX, DUMP, DBG><<<dim3(grid), dim3(G::NT), lds_bytes, a.s>>>(a.x, a.z, a.ldj, a.ws, a.B, a.xbs, a.dbg, 0, a.sb, a.tp);
    return 0;
}
// the specialist coupling (CTX != 0) never sits behind a squeeze: only its SQ = false form is built
template <class G, int CTX = 0, bool DUMP = false, bool DBG = false>
int launch_step(const StepArgs& a) {
    if constexpr (CTX == 0) { if (a.sq) return launch_step_sq<G, true, CTX, DUMP, DBG>(a); }
    return launch_step_sq<G, false, CTX, DUMP, DBG>(a);
}

template <class G, bool SQ>
int launch_step_level_sq(const StepArgs& a, const WsChain& wc, int n) {
    constexpr size_t lds_bytes = (size_t)G::LDS_FLOATS * sizeof(float);
    if (lds_bytes > 64 * 1024) {
        static std::atomic<uint64_t> raised{0};
        if (int rc_ = cf_raise_dynamic_lds((const void*)k_flow_step_level<G, SQ>, 160 * 1024, raised, __func__)) return rc_;
    }
    k_flow_step_level<G, SQ><<<dim3((a.B + G::SPW - 1) / G::SPW), dim3(256), lds_bytes, a.s>>>(a.x, a.z, a.ldj, wc, n, a.B, a.xbs);
    return 0;
}
template <class G>
int launch_step_level(const StepArgs& a, const WsChain& wc, int n) {
    return a.sq ? launch_step_level_sq<G, true>(a, wc, n) : launch_step_level_sq<G, false>(a, wc, n);
}

}  // namespace
