// Shared device code of the fused flow-step kernels (forward, inverse, backward): compile-time geometry,
// MFMA operand pipeline, wave-local staging, the conditioner (phases 1-3).  Included by cf_step_fwd.h,
// cf_step_inv.h, cf_step_dispatch.h and cf_step_bwd.h; everything lives in an anonymous namespace of
// the including translation unit.
#pragma once
#include <type_traits>
#include "cf_common.h"
#include <math.h>

namespace {


typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWaves = 4;              // waves per workgroup of every geometry that does not say otherwise (Geo::WAVES)

// ---- compile-time geometry of one supported shape ------------------------------------------------
// PIPE_: form of phase 2, the 3x3 (0 = compiler-scheduled per-tap loop, 1 = explicit two-stage operand pipeline, 2 = all nine
// taps unrolled with precomputed row / column offset parts, 3 = Winograd F(2x2,3x3): winograd_phase2)
// ABL_: timing-only ablations for tools/step_bench.py (1 = phase-2 operands are constants: no LDS / L2 loads there)
// PATCH_: (backward) every row of an LDS plane carries, behind its PIX pixel columns, the fold sums of the transposed
// reflect-padded 3x3 (cf_step_bwd.h): PP slots per sample + one zero slot; RS = row stride of all LDS planes.
template <int C_, int H_, int W_, int SPW_, int PIPE_ = 1, int ABL_ = 0, int PATCH_ = 0>
struct Geo {
    static constexpr int C = C_, H = H_, W = W_, SPW = SPW_, PIPE = PIPE_, ABL = ABL_, PATCH = PATCH_;
    // PIPE == 6 at 4x4 with 16 samples: every column tile of 16 output tiles has ONE tile row, and a wave leaves out the vertical
    // index whose two patch rows reflection makes the same row (winograd24_phase2, "zero skip"); on 8 waves
    static constexpr bool ZSKIP = PIPE_ == 6 && H_ == 4 && SPW_ == 16;
    // waves per workgroup (NT threads): a property of the geometry (not a template parameter: the kernels' names stay what they were)
    static constexpr int WAVES = ZSKIP ? 8 : kWaves, NT = 64 * WAVES;
    static constexpr int HW = H * W;
    static constexpr int PIX = SPW * HW;              // pixels per workgroup
    static constexpr int HALF = C / 2;                // conditioner channels
    static constexpr int HID = 2 * C;                 // hidden width of the coupling net
    static constexpr int NPT = PIX / 32;              // 32-pixel tiles per workgroup
    static constexpr int PTW = NPT / WAVES;           // pixel tiles per wave
    static constexpr int HP = HALF <= 16 ? 16 : 32;   // packed rows per channel half
    static constexpr int R03 = 2 * HP;                // packed rows of the C-channel results (y, h)
    static constexpr int RT03 = R03 / 32;
    static constexpr int RT1 = (HID + 31) / 32;       // row tiles of the hidden planes
    static constexpr int R1 = RT1 * 32;
    // k-steps (2 k per MFMA) and 4-step groups of every contraction
    static constexpr int KS0 = C / 2, KS1 = HALF / 2, KS3 = HID / 2;
    static constexpr int NG0 = (KS0 + 3) / 4, NG1 = (KS1 + 3) / 4, NG3 = (KS3 + 3) / 4;
    static constexpr int NCG = HID / 8;               // groups per 3x3 tap
    static constexpr int NG2 = 9 * NCG;
    // workspace layout (floats)
    static constexpr int OFF_B0 = 4, OFF_B1 = OFF_B0 + R03, OFF_B2 = OFF_B1 + R1, OFF_B3 = OFF_B2 + R1;
    static constexpr int OFF_A0 = OFF_B3 + R03;
    static constexpr int OFF_A1 = OFF_A0 + NG0 * RT03 * 256;
    static constexpr int OFF_A2 = OFF_A1 + NG1 * RT1 * 256;
    static constexpr int OFF_A3 = OFF_A2 + NG2 * RT1 * 256;
    // 16-row phases on v_mfma_f32_16x16x4_f32 (k_flow_step_small: C <= 16 on 16x16 images, one sample per workgroup).
    // With <= 16 real output rows a 32x32x2 tile spends half (or three quarters) of its cycles on padding rows; the
    // 16x16x4 form has the same flop/cycle and no padding.  Extra packed operands, 4 k-steps (16 k) per float4 group:
    //   S0 = e^{-logs} Wm (rows: packed y0 / y1), S3 = NN.4 (rows: packed t / raw); when the hidden planes are one
    //   16-row tile too (C = 8): S1 = NN.0, S2 = NN.2 (9 taps).  SB0 / SB3: the 16 packed-row biases.
    static constexpr bool SMALL = (H == 16 && W == 16 && SPW == 1 && C <= 16);
    static constexpr bool HID16 = SMALL && HID == 16;
    static constexpr int SG0 = (C + 15) / 16, SG3 = (HID + 15) / 16, SG1 = (HALF + 15) / 16;
    static constexpr int OFF_SB0 = OFF_A3 + NG3 * RT03 * 256;
    static constexpr int OFF_SB3 = OFF_SB0 + (SMALL ? 16 : 0);
    static constexpr int OFF_SA0 = OFF_SB3 + (SMALL ? 16 : 0);
    static constexpr int OFF_SA3 = OFF_SA0 + (SMALL ? SG0 * 256 : 0);
    static constexpr int OFF_SA1 = OFF_SA3 + (SMALL ? SG3 * 256 : 0);
    static constexpr int OFF_SA2 = OFF_SA1 + (HID16 ? SG1 * 256 : 0);
    // Winograd F(2x2,3x3) form of the 3x3 (PIPE == 3, winograd_phase2 below): U = G w G^T for the 16 positions, packed as
    // 16x16x4 A fragments: [position][16-row tile][group of 4 k-steps][lane][4]
    // PIPE == 6: Winograd F(2x4, 3x3) on the 4x4 and 8x8 levels (winograd24_phase2): 24 products per 2x4 output tile instead of 2 x 16
    static constexpr bool W24 = (PIPE_ == 6);
    // (PIPE == 4 / 5 were two forms of the 16x16 level on the 16-bit matrix cores: removed)
    static constexpr bool WINO = (PIPE_ == 3 || W24);
    static constexpr int RT16 = HID / 16, KG4 = HID / 16;         // row tiles / k-step groups of the 16x16x4 products over HID
    static constexpr int OFF_AW = OFF_SA2 + (HID16 ? 9 * 256 : 0);
    // one-sample-per-workgroup form of the 4x4 level for small batches (k_flow_step_rs16, cf_step_rs.h): 16x16x4 A fragments
    // of all four products in NATURAL row order, [row tile][group of 4 k-steps][lane][4], + their biases
    static constexpr bool RS16 = (C == 64 && H == 4 && W == 4);
    static constexpr int OFF_RB0 = OFF_AW + 16 * HID * HID, OFF_RB1 = OFF_RB0 + C, OFF_RB2 = OFF_RB1 + HID, OFF_RB3 = OFF_RB2 + HID;
    static constexpr int OFF_RA0 = OFF_RB3 + C, OFF_RA1 = OFF_RA0 + (C / 16) * (C / 16) * 256;
    static constexpr int OFF_RA2 = OFF_RA1 + (HID / 16) * (HALF / 16) * 256, OFF_RA3 = OFF_RA2 + (HID / 16) * 9 * (HID / 16) * 256;
    static constexpr int R16_END = OFF_RA3 + (C / 16) * (HID / 16) * 256;
    static constexpr int WS_END0 = RS16 ? R16_END : OFF_AW + 16 * HID * HID;
    // Winograd-domain weights of the F(2x4, 3x3) form (4x4 and 8x8 images only): U = G2 w G4^T for the 4 x 6 positions, packed as
    // the 16 positions of the F(2x2) form: [position xi * 6 + nu][16-row tile][group of 4 k-steps][lane][4]
    static constexpr bool HAS_W24 = (H == 4 && W == 4) || (H == 8 && W == 8);
    static constexpr int OFF_AW24 = WS_END0;
    static constexpr int WS_FLOATS = OFF_AW24 + (HAS_W24 ? 24 * HID * HID : 0);
    static constexpr int PP = 2 * W + 2 * H + 4;      // fold slots per sample: 2 patched rows, 2 patched columns, 4 corners
    static constexpr int RS = PATCH ? ((PIX + SPW * PP + 1 + 3) & ~3) : PIX;
    // C = 8 (HID = 16) in the Winograd form: all 16 Winograd-domain weight matrices are 16 KB - staged into LDS once per workgroup
    // (LDS_W floats behind the planes) instead of streamed per wave through L1 (that delivery costs 6.7 % of the level:
    // -DCF_ABL_FIXEDW); the larger levels fill their LDS with planes
#ifndef CF_WINO_LDSW
#define CF_WINO_LDSW 1
#endif
    static constexpr int LDS_W = (CF_WINO_LDSW && PIPE_ == 3 && HID == 16 && H == 16 && W == 16 && SPW == 1) ? 16 * HID * HID : 0;
    static constexpr int LDS_FLOATS = (HALF + HID) * RS + LDS_W;
    // waves per SIMD the register allocator must leave room for = workgroups per CU the LDS footprint admits
    static constexpr int MINW = (160 * 1024) / (LDS_FLOATS * 4) >= 4 ? 4 : ((160 * 1024) / (LDS_FLOATS * 4) >= 2 ? 2 : 1);
    static_assert(PIX % 128 == 0 && PTW >= 1 && NPT % WAVES == 0, "workgroup must own a multiple of 128 pixels");
    static_assert(!W24 || (H == 4 && W == 4 && SPW == 8) || (H == 8 && W == 8 && SPW == 4) || ZSKIP,
                  "F(2x4, 3x3): 4x4 images, 8 samples = one column tile of 16 output tiles; 8x8 images, 4 samples = two column tiles");
    static_assert(!ZSKIP || (W == 4 && WAVES == 8 && C == 64), "zero skip: 16 samples of the 4x4 level on 8 waves, the whole LDS");
    static_assert(HID % 8 == 0 && C % 4 == 0, "channel counts must fill whole k-steps");
    static_assert((HW & (HW - 1)) == 0 && (W & (W - 1)) == 0, "power-of-two images");
};

// geometries whose kernels read their per-lane address words from a compile-time table (kLaneTab below; each passed the per-level
// gate of profiles/lane_tables.md); all others derive them
template <class G> constexpr bool kLaneTabW24 = G::W24 && G::H == 8;
template <class G> constexpr bool kLaneTabW22 = G::PIPE == 3 && G::SMALL && G::C == 16;

// packed row p of a C-channel result -> channel, or -1 for a padding row.  First-half channels sit
// in rows [0, HALF), second-half channels in rows [HP, HP + HALF): t / log_s / x1 of one channel
// then share a lane and differ by a fixed register offset.
template <class G> __host__ __device__ constexpr int chan_of_row(int p) {
    return ((p % G::HP) < G::HALF) ? (p / G::HP) * G::HALF + (p % G::HP) : -1;
}

// 16-row packing of the 16x16x4 phases: row 4g + j (g = lane >> 4 owns it in the result tile): j = 0,1 -> first-half
// channel 2g + j, j = 2,3 -> second-half channel HALF + 2g + (j - 2): t / raw / y1 of one channel again share a lane.
template <class G> __host__ __device__ constexpr int chan_of_row16(int p) {
    return (2 * (p >> 2) + (p & 1) < G::HALF) ? ((p & 2) ? G::HALF : 0) + 2 * (p >> 2) + (p & 1) : -1;
}

// ---- helpers -----------------------------------------------------------------------------------------
// accumulator tile initialised with the per-row bias: row(r, lk) = (r&3) + 8*(r>>2) + 4*lk
__device__ __forceinline__ f32x16 bias_tile(const float* __restrict__ bias32, int lk) {
    f32x16 a;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(bias32 + 8 * q + 4 * lk);
        a[4 * q + 0] = v.x; a[4 * q + 1] = v.y; a[4 * q + 2] = v.z; a[4 * q + 3] = v.w;
    }
    return a;
}
__device__ __forceinline__ int tile_row(int r, int lk) { return (r & 3) + 8 * (r >> 2) + 4 * lk; }
// ReLU as ONE integer max on the bit pattern (negative floats are negative integers; -0 -> +0).  fmaxf(x, 0) costs two
// VALU instructions here (hipcc quiets a possible sNaN with v_max x,x first), and in the MFMA kernels every VALU
// instruction is time the matrix pipe of that SIMD stands still.
__device__ __forceinline__ float cf_relu(float x) { return __int_as_float(max(__float_as_int(x), 0)); }
// log_s = 2 tanh(raw / 2) = 2 - 4 / (e^raw + 1)   (coupling.py:55-56) on the hardware exp / rcp path (v_exp_f32, v_rcp_f32:
// 1 ulp each): |abs err| <= ~3e-7 per element, i.e. ~1e-8 bits/dim after the per-sample sum (tolerance 1e-5; measured on
// the stress fixtures with |raw| up to 25: tests/test_gpu_parity.py::test_e2e_stress_regimes).  e^raw = inf gives 2,
// e^raw = 0 gives -2 exactly.  (`__fdividef` is an IEEE division on this toolchain: ~10 more VALU per element.)
__device__ __forceinline__ float cf_log_scale(float raw) { return fmaf(-4.0f, __builtin_amdgcn_rcpf(__expf(raw) + 1.0f), 2.0f); }
__device__ __forceinline__ float f4e(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

// Operands of one 4-k-step group: RT weight fragments (one 16-byte load each) and 4*PTW activation values.
template <int RT, int PTW>
struct GroupOps {
    float4 a[RT];
    float b[4][PTW];
};

template <int RT, int PTW>
__device__ __forceinline__ void group_mma(f32x16 (&acc)[RT][PTW], const GroupOps<RT, PTW>& o, int nsteps) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (e < nsteps) {
#pragma unroll
            for (int q = 0; q < PTW; ++q)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
                    acc[rt][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(f4e(o.a[rt], e), o.b[e][q], acc[rt][q], 0, 0, 0);
        }
    }
}

// Packed weight fragments are fetched through a buffer resource: `buffer_load_dwordx4 v, v_lane16, s[rsrc], s_off offen`
// takes the group / row-tile / tap offset as a SCALAR, so no per-load 64-bit vector address arithmetic sits between the
// MFMAs (the flat form costs v_lshl_add_u64 / v_add_co / v_addc per fragment).
typedef __amdgpu_buffer_rsrc_t ws_rsrc_t;
__device__ __forceinline__ ws_rsrc_t ws_rsrc(const float* ws, int floats) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ws), 0, floats * 4, 0x00020000);
}
// fragment at float offset `foff` (wave-uniform) + this lane's 16 bytes
__device__ __forceinline__ float4 ws_frag(ws_rsrc_t rs, int lane, int foff) {
    typedef int i32x4_t __attribute__((ext_vector_type(4)));
    const i32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 16, foff * 4, 0);
    return make_float4(__int_as_float(v.x), __int_as_float(v.y), __int_as_float(v.z), __int_as_float(v.w));
}

// One dense phase whose B operand is an LDS plane [k][PIX]:  acc[rt][q] += A_frag * plane
//   KS real k-steps, NG groups of 4, RT row tiles, frags = packed A of this phase.
// Software pipeline: the operands of group g+1 are requested BEFORE the MFMAs of group g are issued
// (sched_barrier pins the loads there: left alone, hipcc sinks them next to their first use and every
// group then stalls on an L2 round trip).
template <class G, int KS, int NG, int RT, class FRAG>
__device__ __forceinline__ void dense_phase_impl(f32x16 (&acc)[RT][G::PTW], FRAG frag,
                                                 const float* __restrict__ plane, const int (&pix)[G::PTW], int lane) {
    const int lk = lane >> 5;
    cf_wave_sync();                      // the operand plane was written by other lanes of this wave
    GroupOps<RT, G::PTW> ops[2];
    auto load = [&](int g, GroupOps<RT, G::PTW>& o) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) o.a[rt] = frag(g * RT + rt);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int q = 0; q < G::PTW; ++q)
                o.b[e][q] = (4 * g + e < KS) ? plane[(2 * (4 * g + e) + lk) * G::RS + pix[q]] : 0.f;
    };
    load(0, ops[0]);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        if (g + 1 < NG) load(g + 1, ops[(g + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        group_mma<RT, G::PTW>(acc, ops[g & 1], KS - 4 * g);
    }
}
template <class G, int KS, int NG, int RT>
__device__ __forceinline__ void dense_phase(f32x16 (&acc)[RT][G::PTW], const float4* __restrict__ frags,
                                            const float* __restrict__ plane, const int (&pix)[G::PTW], int lane) {
    dense_phase_impl<G, KS, NG, RT>(acc, [&](int i) { return frags[i * 64 + lane]; }, plane, pix, lane);
}
// same, fragments through a buffer resource at float offset `foff`
template <class G, int KS, int NG, int RT>
__device__ __forceinline__ void dense_phase(f32x16 (&acc)[RT][G::PTW], ws_rsrc_t rs, int foff,
                                            const float* __restrict__ plane, const int (&pix)[G::PTW], int lane) {
    dense_phase_impl<G, KS, NG, RT>(acc, [&](int i) { return ws_frag(rs, lane, foff + i * 256); }, plane, pix, lane);
}

// Streaming accesses of the step kernels (x is read once, z written once per step): non-temporal, so that they do not displace
// the weight fragments every workgroup re-reads from L1 / L2 (-DCF_STREAM_NT=0: plain accesses, A/B)
#ifndef CF_STREAM_NT
#define CF_STREAM_NT 1
#endif
__device__ __forceinline__ float4 cf_ld_stream(const float4* p) {
#if CF_STREAM_NT
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    return make_float4(v[0], v[1], v[2], v[3]);
#else
    return *p;
#endif
}
__device__ __forceinline__ float cf_ldf_stream(const float* p) {
#if CF_STREAM_NT
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}
__device__ __forceinline__ void cf_st_stream(float4* p, const float4 v) {
#if CF_STREAM_NT
    __builtin_nontemporal_store(f32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<f32x4*>(p));
#else
    *p = v;
#endif
}

// ---- wave-local staging of activations with 16-byte global accesses ---------------------------------
// A wave owns WPX = 32*PTW pixel columns.  Item n = i*64 + lane enumerates its C x WPX block of x.
template <class G, bool SQ>
__device__ __forceinline__ void x_load(float4 (&xr)[G::C * G::PTW / 8], const float* __restrict__ x, int64_t xbs,
                                       int tile, int B, int wave, int lane) {
    constexpr int WPX = 32 * G::PTW, HW = G::HW, W = G::W;
    const int tb0 = tile * G::SPW;
#pragma unroll
    for (int i = 0; i < G::C * G::PTW / 8; ++i) {
        const int n = i * 64 + lane;
        if constexpr (!SQ) {
            const int ch = n / (WPX / 4), col = wave * WPX + 4 * (n % (WPX / 4));
            const int b = min(tb0 + col / HW, B - 1);
            xr[i] = cf_ld_stream(reinterpret_cast<const float4*>(x + (int64_t)b * xbs + ch * HW + col % HW));
        } else {
            // un-squeezed row (2y+i1), 4 consecutive floats = channels (4c'+2i1, +1) of squeezed pixels (x, x+1)
            const int cp = n / (WPX / 2), col = wave * WPX + 2 * (n % (WPX / 2));
            const int b = min(tb0 + col / HW, B - 1);
            const int p = col % HW, yy = p / W, xx = p % W;
            xr[i] = cf_ld_stream(reinterpret_cast<const float4*>(x + (int64_t)b * xbs + (cp >> 1) * 4 * HW + (2 * yy + (cp & 1)) * 2 * W + 2 * xx));
        }
    }
}

template <class G, bool SQ>
__device__ __forceinline__ void x_to_lds(const float4 (&xr)[G::C * G::PTW / 8], float* __restrict__ plane, int wave, int lane) {
    constexpr int WPX = 32 * G::PTW, PIX = G::RS;      // row stride of the plane
#pragma unroll
    for (int i = 0; i < G::C * G::PTW / 8; ++i) {
        const int n = i * 64 + lane;
        if constexpr (!SQ) {
            const int ch = n / (WPX / 4), col = wave * WPX + 4 * (n % (WPX / 4));
            *reinterpret_cast<float4*>(&plane[ch * PIX + col]) = make_float4(xr[i].x, xr[i].y, xr[i].z, xr[i].w);
        } else {
            const int cp = n / (WPX / 2), col = wave * WPX + 2 * (n % (WPX / 2));
            *reinterpret_cast<float2*>(&plane[(2 * cp) * PIX + col]) = make_float2(xr[i].x, xr[i].z);
            *reinterpret_cast<float2*>(&plane[(2 * cp + 1) * PIX + col]) = make_float2(xr[i].y, xr[i].w);
        }
    }
    cf_wave_sync();
}

// write NROWS channel rows (channels ch0 .. ch0+NROWS-1 of a (B,C,H,W) tensor) from an LDS plane [row][PIX]
// (this wave's columns), 16 bytes per lane
template <class G, int NROWS>
__device__ __forceinline__ void rows_store(float* __restrict__ z, const float* __restrict__ plane, int tb0, int ch0, int B,
                                           int wave, int lane) {
    constexpr int WPX = 32 * G::PTW, HW = G::HW, PIX = G::RS, C = G::C;
    cf_wave_sync();                      // rows written by other lanes of this wave
#pragma unroll
    for (int i = 0; i < (NROWS * G::PTW + 7) / 8; ++i) {
        const int n = i * 64 + lane;
        const int idx = n / (WPX / 4), col = wave * WPX + 4 * (n % (WPX / 4));
        const int b = tb0 + col / HW;
        if (idx < NROWS && b < B)
            cf_st_stream(reinterpret_cast<float4*>(z + (int64_t)b * C * HW + (int64_t)(ch0 + idx) * HW + col % HW),
                         *reinterpret_cast<const float4*>(&plane[idx * PIX + col]));
    }
    cf_wave_sync();                      // ... read back before anyone reuses the words
}
template <class G>
__device__ __forceinline__ void z_store(float* __restrict__ z, const float* __restrict__ plane, int tb0, int ch0, int B,
                                        int wave, int lane) {
    rows_store<G, G::HALF>(z, plane, tb0, ch0, B, wave, lane);
}

// rows_store for a target tensor with CT channels per sample, and its inverse (global -> this wave's columns of a plane).
// Both go through a buffer resource that covers exactly the VALID samples of this workgroup's tile of the tensor: the
// per-lane byte offset is one 32-bit register for every plane of that shape (item i adds a constant, which travels in the
// scalar offset operand), there is no 64-bit address arithmetic and no `b < B` compare - an access beyond the last sample
// is out of range for the resource: stores are dropped and loads return 0 by the hardware's range check.
template <class G, int CT>
__device__ __forceinline__ ws_rsrc_t tile_rsrc(const float* t, int tb0, int B) {
    const int nb = min(B - tb0, G::SPW);
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(t + (int64_t)tb0 * CT * G::HW), 0, nb * CT * G::HW * 4, 0x00020000);
}
// 16-byte store through a buffer resource with a SCALAR offset, as ONE unit with a wait state behind it.  Measured on
// gfx950: the VGPRs holding the data of a `buffer_store_dwordx4 ... s_off offen` must not be written by the VALU
// instruction right behind it (hipcc places one there when the registers become free - it treats a store with a
// register soffset as hazard-free - and the stored rows then carry the new register contents in some lanes:
// per-call checks of the weight-gradient inputs found 64-bit addresses inside the g_h2 plane; reproducer: tools/micro/store_hazard.hip).  Inline asm: the compiler cannot slide anything
// between the store and its s_nop.
typedef int cf_i32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ cf_i32x4 tile_rsrc_words(const float* base, int bytes) {
    const uint64_t p = reinterpret_cast<uint64_t>(base);
    return cf_i32x4{(int)(uint32_t)p, (int)((uint32_t)(p >> 32) & 0xffffu), bytes, 0x00020000};
}
__device__ __forceinline__ void tile_store_b128(const cf_i32x4 rs, int voff, int soff, const float4 v) {
    typedef float f32x4s __attribute__((ext_vector_type(4)));
    const f32x4s d = {v.x, v.y, v.z, v.w};
#if CF_STREAM_NT      // planes of the tape / gradient planes: written once, read by another kernel - non-temporal, as the z rows
    asm volatile("buffer_store_dwordx4 %0, %1, %2, %3 offen nt\n\ts_nop 1" : : "v"(d), "v"(voff), "s"(rs), "s"(soff) : "memory");
#else
    asm volatile("buffer_store_dwordx4 %0, %1, %2, %3 offen\n\ts_nop 1" : : "v"(d), "v"(voff), "s"(rs), "s"(soff) : "memory");
#endif
}

template <class G, int NROWS, int CT>
__device__ __forceinline__ void rows_store_t(float* __restrict__ dst, const float* __restrict__ plane, int tb0, int B,
                                             int wave, int lane) {
    constexpr int WPX = 32 * G::PTW, HW = G::HW, PIX = G::RS, RPI = 256 / WPX;      // rows per item of 64 lanes x 16 bytes
    const cf_i32x4 rs = tile_rsrc_words(dst + (int64_t)tb0 * CT * HW, min(B - tb0, G::SPW) * CT * HW * 4);
    const int idx0 = lane / (WPX / 4), col = wave * WPX + 4 * (lane % (WPX / 4));
    const int voff = ((col / HW) * CT * HW + idx0 * HW + col % HW) * 4;
    cf_wave_sync();
#ifdef CF_ABL_NOSTORE                    // timing-only ablation (tools/dev/make_abl.py): no plane stores
    if (tb0 >= 0) return;
#endif
#pragma unroll
    for (int i = 0; i < (NROWS + RPI - 1) / RPI; ++i) {
        if (NROWS % RPI == 0 || idx0 + i * RPI < NROWS) {
            const float4 v = *reinterpret_cast<const float4*>(&plane[(idx0 + i * RPI) * PIX + col]);
            tile_store_b128(rs, voff, i * RPI * HW * 4, v);
        }
    }
    cf_wave_sync();
}
// the C rows of `plane` (this wave's own columns) to dst in the layout of the tensor BEFORE Squeeze((2,2)) (squeeze.py:10-11):
// squeezed channel c = 4 q + 2 dy + dx at pixel (y, x) is element (q, 2 y + dy, 2 x + dx) of the (C/4, 2H, 2W) sample.  A
// lane takes the channel pair (2 j, 2 j + 1) = (dx 0, 1) of q = j >> 1, dy = j & 1 at 4 pixels of one image row: 8
// consecutive floats of the destination, two 16-byte stores.
template <class G>
__device__ __forceinline__ void rows_store_unsq(float* __restrict__ dst, const float* __restrict__ plane, int tb0, int B,
                                                int wave, int lane) {
    constexpr int WPX = 32 * G::PTW, HW = G::HW, W = G::W, PIX = G::RS, C = G::C, Q4 = WPX / 4;
    static_assert(C % 4 == 0 && W % 4 == 0, "channel quadruples, 4 pixels of one image row");
    cf_wave_sync();
    for (int it = lane; it < (C / 2) * Q4; it += 64) {
        const int j = it / Q4, col = wave * WPX + 4 * (it - j * Q4);
        const int smp = tb0 + col / HW, p = col % HW, yy = p / W, xx = p - yy * W;
        if (smp < B) {
            const float4 a = *reinterpret_cast<const float4*>(&plane[(2 * j) * PIX + col]);
            const float4 b = *reinterpret_cast<const float4*>(&plane[(2 * j + 1) * PIX + col]);
            float* d = dst + (int64_t)smp * C * HW + (j >> 1) * 4 * HW + (2 * yy + (j & 1)) * 2 * W + 2 * xx;
            *reinterpret_cast<float4*>(d) = make_float4(a.x, b.x, a.y, b.y);
            *reinterpret_cast<float4*>(d + 4) = make_float4(a.z, b.z, a.w, b.w);
        }
    }
    cf_wave_sync();
}
template <class G, int NROWS, int CT>
__device__ __forceinline__ void rows_load_t(const float* __restrict__ src, float* __restrict__ plane, int tb0, int B,
                                            int wave, int lane) {
    typedef int i32x4_t __attribute__((ext_vector_type(4)));
    constexpr int WPX = 32 * G::PTW, HW = G::HW, PIX = G::RS, RPI = 256 / WPX;
    const ws_rsrc_t rs = tile_rsrc<G, CT>(src, tb0, B);
    const int idx0 = lane / (WPX / 4), col = wave * WPX + 4 * (lane % (WPX / 4));
    const int voff = ((col / HW) * CT * HW + idx0 * HW + col % HW) * 4;
    cf_wave_sync();                      // earlier readers of these words (other lanes) are done
#pragma unroll
    for (int i = 0; i < (NROWS + RPI - 1) / RPI; ++i) {
        if (NROWS % RPI == 0 || idx0 + i * RPI < NROWS) {
            const i32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, i * RPI * HW * 4, 0);
            *reinterpret_cast<float4*>(&plane[(idx0 + i * RPI) * PIX + col]) =
                make_float4(__int_as_float(v.x), __int_as_float(v.y), __int_as_float(v.z), __int_as_float(v.w));
        }
    }
    cf_wave_sync();
}

// training tape of a step (forward with DUMP writes, backward with TAPED reads):
//   y0 (B, C/2, HW), h1 / h2 (B, 2C, HW; post-ReLU hidden planes of the conditioner): operands of the weight-gradient GEMMs;
//   ls, y1 (B, C/2, HW): log-scale and the second half of the step's Conv1x1+ActNorm output - with them the backward
//   kernel needs neither the step input nor a recompute of the first and last 1x1;
//   m1 / m2: the ReLU masks of h1 / h2 as bit words in the accumulator layout of the 32x32x2 tiles: word
//   [(T * RT1 + rt) * 64 + lane], T = global 32-pixel tile (sample-major pixel index / 32), bit r = row rt*32 + tile_row(r, lane>>5)
//   of pixel 32 T + (lane & 31).  Sized for the batch rounded up to 16 samples (cf_flow_step_tape_aux_bytes).
struct StepTape {
    float* y0;
    float* h1;
    float* h2;
    float* ls;
    float* y1;
    unsigned* m1;
    unsigned* m2;
};
constexpr StepTape kNoTape{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
// host: the four small tape items live in ONE caller-provided buffer `aux` = [ls | y1 | m1 | m2]
inline int64_t tape_mask_words(int B, int C, int H, int W) {
    return (int64_t)((B + 15) & ~15) * H * W / 32 * ((2 * C + 31) / 32) * 64;
}
inline int64_t tape_aux_bytes(int B, int C, int H, int W) {
    return (2 * (int64_t)B * (C / 2) * H * W + 2 * tape_mask_words(B, C, H, W)) * 4;
}
inline StepTape make_tape(float* y0, float* h1, float* h2, void* aux, int B, int C, int H, int W) {
    const int64_t nh = (int64_t)B * (C / 2) * H * W, nm = tape_mask_words(B, C, H, W);
    float* a = (float*)aux;
    return StepTape{y0, h1, h2, a, a + nh, (unsigned*)(a + 2 * nh), (unsigned*)(a + 2 * nh) + nm};
}

// ReLU mask words of RT x PTW accumulator tiles (pre- or post-ReLU values: the bit is `value > 0` either way)
template <class G, int RT>
__device__ __forceinline__ void mask_store(unsigned* __restrict__ m, const f32x16 (&acc)[RT][G::PTW], int tile, int wave, int lane) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int q = 0; q < G::PTW; ++q) {
            unsigned b = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) b |= (acc[rt][q][r] > 0.f ? 1u : 0u) << r;
            m[((int64_t)(tile * G::NPT + wave * G::PTW + q) * RT + rt) * 64 + lane] = b;
        }
}

// ---- Winograd F(2x2,3x3) form of the reflect-padded 3x3 (phase 2 of PIPE == 3 geometries) ---------------------------
// The 3x3 holds 72 of the 80 C^2 HW multiply-adds of a step and the exact-fp32 matrix pipe is the bound of the whole path,
// so the way past it is fewer multiplications: per 2x2 output tile and channel pair, 16 products instead of 36,
//     Y = A^T [ sum_ci U[ci] (.) (B^T d[ci] B) ] A,     U = G w G^T (packed once, fp64 -> fp32, k_step_pack),
// d = the 4x4 input patch of the tile (reflect-padded), B^T = [[1,0,-1,0],[0,1,1,0],[0,-1,1,0],[0,1,0,-1]],
// A^T = [[1,1,1,0],[0,1,-1,-1]].  All entries are 0 / +-1 (the 1/2 of G lives in the packed weights): the transforms are
// additions, the error of the fp32 result is ~1.6x that of the direct sum (tests/dev_winograd_numerics.py: bits/dim of
// every end-to-end fixture unchanged to its last fp32 digit).
// Mapping: the 16 "positions" (xi, nu) are 16 independent (HID x HID) x (HID x tiles) products on v_mfma_f32_16x16x4_f32;
// a wave owns the 16 tiles (= 64 output pixels) of its own pixel columns and ALL output rows, so the B operand - one
// Winograd-domain value per lane and k-step = 4 LDS reads + 3 additions - serves HID/16 MFMAs, and h2 goes straight back to
// this wave's columns.  The output transform is folded position by position into the four Y accumulators (+-M).
// h1 layout (written by phase 1 of the same geometry): pixel (s, y, x) of row k sits at
//     k PIX + [ s HW + (y&1) HW/2 + (y>>1) W + (x&1) W/2 + (x>>1) ]  ^  (k&1) W/2
// - rows and columns split by parity, so the stride-2 patch reads of neighbouring tiles are consecutive words, and the
// XOR moves odd rows k to the other column-parity block: the 32 lanes of a half wave (16 tiles x 2 channels) hit 32 banks.
template <class G> __host__ __device__ constexpr int wino_pix(int sHW, int y, int x) {
    int p = sHW + (y & 1) * (G::HW / 2) + (y >> 1) * G::W + (x & 1) * (G::W / 2) + (x >> 1);
    if constexpr (G::HW == 16) p ^= ((p >> 5) & 1) << 3;       // 4x4: four samples per wave - fold the sample bit that would alias
    return p;
}

#ifndef CF_WINO_PEEL
#define CF_WINO_PEEL 1
#endif

// Loop form: the 16 positions run as a RUNTIME loop over xi (row of B^T / A^T on the vertical axis) around the four nu,
// unrolled.  (All 16 unrolled was measured first: 4x the code, and hipcc spilled 50-150 registers at 2-3 workgroups / CU:
// 561 / 448 / 414 us per 16384 samples at C = 16 / 32 / 64 against 447 / 372 / 406 us in this form; direct 3x3: 640 / 618 /
// 620 us.)  What depends on xi is data: the two patch rows (xi = 2 takes them swapped, so that the vertical transform is
// t1 + sigma t2 with sigma = +1 for xi = 1 and -1 otherwise), the fragment offset (a scalar), the coefficients A^T[i][xi].
// Operands of a group of 4 k-steps (RT16 weight fragments from L2, 4 patch values per Winograd-domain operand from LDS,
// k-steps paired so that the additions run as packed fp32) are requested one group ahead - the first group of the next xi
// during the last one of this xi - and sched_barrier keeps hipcc from sinking them to their first use.  k runs in chunks
// of <= 64 channels (outer loop): inside a chunk every operand address is `patch offset + immediate`; the output
// transform is linear, so each chunk's partial M is folded into Y.
// tw (kLaneTabW22 geometries): the words of this thread's table entry (W22Lane), requested by the caller in front of the barrier
// that ends phase 1; the others pass nothing and derive
template <class G>
__device__ __forceinline__ void winograd_phase2(float* __restrict__ lds, const float* __restrict__ wsl, ws_rsrc_t rs, int lane,
                                                     int wave, const int4* tw = nullptr) {
    constexpr int W = G::W, H = G::H, HW = G::HW, PIX = G::PIX, HALF = G::HALF, HID = G::HID, RT16 = G::RT16, KG4 = G::KG4;
    // Ownership.  PTW even: a wave takes the NT = PTW / 2 column tiles (16 output tiles = 64 pixels each) of its own pixel
    // columns and ALL output rows.  PTW = 1 (128 pixels per workgroup: half the LDS, two workgroups per CU): two waves share a
    // column tile and split the output ROWS (RSPLIT = 2) - the Winograd-domain operands are formed twice, h2 needs a workgroup
    // barrier before phase 3, but a second workgroup per CU covers the stalls of a lone wave per SIMD (C = 64: 406 -> see DESIGN).
    constexpr int RSPLIT = G::PTW == 1 ? 2 : 1, NT = G::PTW * RSPLIT / 2, NCW = 4 / RSPLIT, RTW = RT16 / RSPLIT;
    static_assert((G::PTW == 1 || G::PTW % 2 == 0) && HID % 16 == 0 && RT16 % RSPLIT == 0, "column tiles of 16 output tiles");
    const int cw = RSPLIT == 1 ? wave : wave % NCW;           // this wave's column-tile group ...
    const int rt0 = RSPLIT == 1 ? 0 : __builtin_amdgcn_readfirstlane((wave / NCW) * RTW);      // ... and first 16-row tile (a constant / a scalar)
    typedef float f32x2w __attribute__((ext_vector_type(2)));
    float* H1 = lds + HALF * PIX;
    const int l15 = lane & 15, lg = lane >> 4;
    constexpr int TPS = HW / 4;
    int smp[NT], ty[NT], tx[NT], rpart[NT][4], cpart[NT][4], dsto = 0;
    if constexpr (kLaneTabW22<G>) {
        static_assert(NT == 1 && RSPLIT == 1, "W22Lane holds one column tile");
        const int4 t0 = tw[0], t1 = tw[1];
        rpart[0][0] = t0.x; rpart[0][1] = t0.y; rpart[0][2] = t0.z; rpart[0][3] = t0.w;
        cpart[0][0] = t1.x; cpart[0][1] = t1.y; cpart[0][2] = t1.z; cpart[0][3] = t1.w;
        dsto = tw[2].z;
    } else
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
        const int tg = (cw * NT + ct) * 16 + l15, ti = tg % TPS;
        smp[ct] = tg / TPS; ty[ct] = ti / (W / 2); tx[ct] = ti % (W / 2);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            int yy = 2 * ty[ct] - 1 + a, xx = 2 * tx[ct] - 1 + a;
            yy = yy < 0 ? -yy : (yy >= H ? 2 * (H - 1) - yy : yy);
            xx = xx < 0 ? -xx : (xx >= W ? 2 * (W - 1) - xx : xx);
            // BYTE offsets: an operand address is then one addition (row part + column part) in front of the ds_read's immediate
            rpart[ct][a] = 4 * (HALF * PIX + lg * PIX + wino_pix<G>(smp[ct] * HW, yy, 0));
            cpart[ct][a] = 4 * ((((xx ^ lg) & 1) * (W / 2)) + (xx >> 1));
        }
    }
    f32x4 Y[NT][2][2][RTW];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int rt = 0; rt < RTW; ++rt) Y[ct][i][j][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
    struct WFrag { float4 a[RTW]; };
    struct WPatch { f32x2w d[NT][2][4]; };
    constexpr int KGC = KG4 < 4 ? KG4 : 4, NCH = KG4 / KGC, NGX = 4 * KGC;       // groups per xi
    static_assert(NGX % 2 == 0, "static ping-pong");
    constexpr int B1[4] = {0, 1, 1, 1}, B2[4] = {2, 2, 2, 3};                       // patch columns of B^T row nu
    constexpr float S1[4] = {1.f, 1.f, -1.f, 1.f}, S2[4] = {-1.f, 1.f, 1.f, -1.f};
    constexpr float AT[2][4] = {{1.f, 1.f, 1.f, 0.f}, {0.f, 1.f, -1.f, -1.f}};
    // ---- column-shared form (HID <= 64: one k-chunk, no row split) ------------------------------------------------------
    // B^T d B for one vertical index xi: A[c] = d[r1][c] + sigma d[r2][c] for the four patch columns c, and the four
    // horizontal positions are  nu 0: A0 - A2,  1: A1 + A2,  2: A2 - A1,  3: A1 - A3.  A1 / A2 of every k-group are kept for
    // the whole xi (2 x 4 values per k-group), A0 / A3 are formed where nu = 0 / 3 uses them: 8 LDS reads + 8 VALU per
    // channel and xi instead of 16 + 12 in the per-position form below, same register footprint (no extra accumulators).
    // At HID = 32 / 16 a transformed operand feeds only 2 / 1 MFMAs: the per-position form kept the CU's LDS pipe 50 / 100 %
    // busy with patch reads (round 2 PMC: SQ_WAIT_INST_LDS 7x the C = 32 level's) and spilled 5-7 registers at 4 workgroups
    // per CU.  Measured (tools/dev/ab_step.py, 65536 samples): C = 8  0.73 -> 0.68 ms, C = 16  1.76 -> 1.64 ms (no spills),
    // C = 32  1.50 -> 1.47 ms.  (Also measured: the same arithmetic on scalar floats with -fno-slp-vectorize, as the
    // micro-architecture guide suggests for VALU beside 16-bit MFMAs - no gain at C = 16, 2 % slower at C = 32 / 64: the fp32
    // MFMA shares the fp32 lanes with the VALU, so what counts here is the NUMBER of vector instructions, and packed ones
    // halve it.)
#ifndef CF_WINO_VF_MAXRT
#define CF_WINO_VF_MAXRT 4
#endif
    constexpr bool VF = RT16 <= CF_WINO_VF_MAXRT && NCH == 1 && RSPLIT == 1;
    if constexpr (VF) {
        const float* base = lds;
        constexpr int frc = G::OFF_AW;
        auto rows_of = [&](int xi, int (&r1)[NT], int (&r2)[NT]) {
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                r1[ct] = xi == 0 ? rpart[ct][0] : (xi == 2 ? rpart[ct][2] : rpart[ct][1]);
                r2[ct] = xi == 2 ? rpart[ct][1] : (xi == 3 ? rpart[ct][3] : rpart[ct][2]);
            }
        };
        // operands of group g = nu KGC + kk: the weight fragments and the raw patch columns the group has to fold
        // (nu 0: columns 0 and 2, nu 1: column 1, nu 2: none, nu 3: column 3); k-steps paired for packed arithmetic
        struct WRaw { f32x2w d[NT][2][2][2]; };               // [ct][slot][row r1 / r2][k-step pair]
        WFrag fa[2];
        WRaw raw[2];
        auto load = [&](int xi, const int (&r1)[NT], const int (&r2)[NT], int g, WFrag& fo, WRaw& o) {
            const int nu = g / KGC, kk = g % KGC;
#ifdef CF_ABL_FIXEDW                       // timing-only probe: every group reads the SAME fragments (L1-resident; wrong results)
            const int fr = frc + (0 * xi * nu * kk) * 256;
#else
            const int fr = frc + ((xi * 4 + nu) * RT16 * KG4 + kk) * 256;
#endif
            if constexpr (G::LDS_W > 0) {            // staged by the kernel (k_flow_step_small) behind the planes, same fragment order
#pragma unroll
                for (int rt = 0; rt < RTW; ++rt)
                    fo.a[rt] = *reinterpret_cast<const float4*>(lds + (HALF + HID) * G::RS + (fr - frc) + (rt0 + rt) * KG4 * 256 + lane * 4);
            } else {
#pragma unroll
                for (int rt = 0; rt < RTW; ++rt) fo.a[rt] = ws_frag(rs, lane, fr + (rt0 + rt) * KG4 * 256);
            }
            constexpr int NC[4] = {2, 1, 0, 1}, C0[4] = {0, 1, 0, 3}, C1[4] = {2, 0, 0, 0};
#pragma unroll
            for (int ct = 0; ct < NT; ++ct)
#pragma unroll
                for (int sl = 0; sl < 2; ++sl)
                    if (sl < NC[nu]) {
                        const int c = sl == 0 ? C0[nu] : C1[nu];
                        const int o1 = r1[ct] + cpart[ct][c], o2 = r2[ct] + cpart[ct][c];
#pragma unroll
                        for (int e2 = 0; e2 < 2; ++e2) {
                            const char* q0 = reinterpret_cast<const char*>(base + (16 * kk + 8 * e2) * PIX);
                            const char* q1 = q0 + 4 * PIX * 4;
                            auto at = [](const char* q, int ob) { return *reinterpret_cast<const float*>(q + ob); };
                            o.d[ct][sl][0][e2] = f32x2w{at(q0, o1), at(q1, o1)};
                            o.d[ct][sl][1][e2] = f32x2w{at(q0, o2), at(q1, o2)};
                        }
                    }
        };
        f32x2w A1[KGC][NT][2], A2[KGC][NT][2];
        int r1[NT], r2[NT], r1n[NT], r2n[NT];
        rows_of(0, r1, r2);
        load(0, r1, r2, 0, fa[0], raw[0]);
        // the vertical coefficients A^T[0][xi] = (1, 1, 1, 0) and A^T[1][xi] = (0, 1, -1, -1): xi = 0 and xi = 3 are peeled so that
        // their zero halves of the output transform are not executed (CF_WINO_PEEL; the loop keeps xi = 1, 2)
        auto xi_body = [&](const int xi, auto has0, auto has1) {
            const int xn = xi < 3 ? xi + 1 : 3;
            rows_of(xn, r1n, r2n);
            const float sigma = xi == 1 ? 1.f : -1.f;
            const float c0 = xi < 3 ? 1.f : 0.f, c1 = xi == 0 ? 0.f : (xi == 1 ? 1.f : -1.f);      // A^T[0][xi], A^T[1][xi]
#pragma unroll
            for (int nu = 0; nu < 4; ++nu) {
                f32x4 M[NT][RTW];
#pragma unroll
                for (int ct = 0; ct < NT; ++ct)
#pragma unroll
                    for (int rt = 0; rt < RTW; ++rt) M[ct][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < KGC; ++kk) {
                    const int g = nu * KGC + kk;
                    if (g + 1 < NGX) load(xi, r1, r2, g + 1, fa[(g + 1) & 1], raw[(g + 1) & 1]);
                    else load(xn, r1n, r2n, 0, fa[0], raw[0]);           // first group of the next xi (after the last xi: harmless)
                    __builtin_amdgcn_sched_barrier(0);
                    const WFrag& oa = fa[g & 1];
                    const WRaw& o = raw[g & 1];
                    f32x2w v[NT][2];
#pragma unroll
                    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
                        for (int e2 = 0; e2 < 2; ++e2) {
                            if (nu == 0) {
                                const f32x2w a0 = o.d[ct][0][0][e2] + sigma * o.d[ct][0][1][e2];
                                A2[kk][ct][e2] = o.d[ct][1][0][e2] + sigma * o.d[ct][1][1][e2];
                                v[ct][e2] = a0 - A2[kk][ct][e2];
                            } else if (nu == 1) {
                                A1[kk][ct][e2] = o.d[ct][0][0][e2] + sigma * o.d[ct][0][1][e2];
                                v[ct][e2] = A1[kk][ct][e2] + A2[kk][ct][e2];
                            } else if (nu == 2) {
                                v[ct][e2] = A2[kk][ct][e2] - A1[kk][ct][e2];
                            } else {
                                const f32x2w a3 = o.d[ct][0][0][e2] + sigma * o.d[ct][0][1][e2];
                                v[ct][e2] = A1[kk][ct][e2] - a3;
                            }
                        }
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int rt = 0; rt < RTW; ++rt)
#pragma unroll
                            for (int ct = 0; ct < NT; ++ct)
                                M[ct][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4e(oa.a[rt], e), v[ct][e >> 1][e & 1], M[ct][rt], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                // Y[i][j] += A^T[i][xi] A^T[j][nu] M
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (AT[j][nu] != 0.f) {
                        const float k0 = c0 * AT[j][nu], k1 = c1 * AT[j][nu];
#pragma unroll
                        for (int ct = 0; ct < NT; ++ct)
#pragma unroll
                            for (int rt = 0; rt < RTW; ++rt) {
                                if constexpr (decltype(has0)::value) Y[ct][0][j][rt] += k0 * M[ct][rt];
                                if constexpr (decltype(has1)::value) Y[ct][1][j][rt] += k1 * M[ct][rt];
                            }
                    }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) { r1[ct] = r1n[ct]; r2[ct] = r2n[ct]; }
        };
        if constexpr (CF_WINO_PEEL == 2) {      // all four bodies (measured: see DESIGN)
            xi_body(0, std::true_type{}, std::false_type{});
            xi_body(1, std::true_type{}, std::true_type{});
            xi_body(2, std::true_type{}, std::true_type{});
            xi_body(3, std::false_type{}, std::true_type{});
        } else if constexpr (CF_WINO_PEEL) {
            xi_body(0, std::true_type{}, std::false_type{});
#pragma unroll 1
            for (int xi = 1; xi < 3; ++xi) xi_body(xi, std::true_type{}, std::true_type{});
            xi_body(3, std::false_type{}, std::true_type{});
        } else {
#pragma unroll 1
            for (int xi = 0; xi < 4; ++xi) xi_body(xi, std::true_type{}, std::true_type{});
        }
    } else {
#pragma unroll 1
    for (int ch = 0; ch < NCH; ++ch) {
        const float* base = lds + ch * (16 * KGC) * PIX;
        const int frc = G::OFF_AW + ch * KGC * 256;
        WFrag fa[2];
        WPatch pd[2];
        auto rows_of = [&](int xi, int (&r1)[NT], int (&r2)[NT]) {          // xi is wave-uniform: selects, not branches
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                r1[ct] = xi == 0 ? rpart[ct][0] : (xi == 2 ? rpart[ct][2] : rpart[ct][1]);
                r2[ct] = xi == 2 ? rpart[ct][1] : (xi == 3 ? rpart[ct][3] : rpart[ct][2]);
            }
        };
        auto load = [&](int xi, const int (&r1)[NT], const int (&r2)[NT], int g, WFrag& fo, WPatch& o) {    // g = nu * KGC + kk (static)
            const int nu = g / KGC, kk = g % KGC;
            const int fr = frc + ((xi * 4 + nu) * RT16 * KG4 + kk) * 256;
#pragma unroll
            for (int rt = 0; rt < RTW; ++rt) fo.a[rt] = ws_frag(rs, lane, fr + (rt0 + rt) * KG4 * 256);
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                const int o11 = r1[ct] + cpart[ct][B1[nu]], o12 = r1[ct] + cpart[ct][B2[nu]];
                const int o21 = r2[ct] + cpart[ct][B1[nu]], o22 = r2[ct] + cpart[ct][B2[nu]];
#pragma unroll
                for (int e2 = 0; e2 < 2; ++e2) {
                    const char* q0 = reinterpret_cast<const char*>(base + (16 * kk + 8 * e2) * PIX);
                    const char* q1 = q0 + 4 * PIX * 4;
                    auto at = [](const char* q, int ob) { return *reinterpret_cast<const float*>(q + ob); };
                    o.d[ct][e2][0] = f32x2w{at(q0, o11), at(q1, o11)}; o.d[ct][e2][1] = f32x2w{at(q0, o12), at(q1, o12)};
                    o.d[ct][e2][2] = f32x2w{at(q0, o21), at(q1, o21)}; o.d[ct][e2][3] = f32x2w{at(q0, o22), at(q1, o22)};
                }
            }
        };
        int r1[NT], r2[NT], r1n[NT], r2n[NT];
        rows_of(0, r1, r2);
        load(0, r1, r2, 0, fa[0], pd[0]);
        auto xi_body = [&](const int xi, auto has0, auto has1) {          // xi = 0 / 3 peeled, as in the column-shared form
            const int xn = xi < 3 ? xi + 1 : 3;
            rows_of(xn, r1n, r2n);
            const float sigma = xi == 1 ? 1.f : -1.f;
            const float c0 = xi < 3 ? 1.f : 0.f, c1 = xi == 0 ? 0.f : (xi == 1 ? 1.f : -1.f);      // A^T[0][xi], A^T[1][xi]
#pragma unroll
            for (int nu = 0; nu < 4; ++nu) {
                f32x4 M[NT][RTW];
#pragma unroll
                for (int ct = 0; ct < NT; ++ct)
#pragma unroll
                    for (int rt = 0; rt < RTW; ++rt) M[ct][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < KGC; ++kk) {
                    const int g = nu * KGC + kk;
                    if (g + 1 < NGX) load(xi, r1, r2, g + 1, fa[(g + 1) & 1], pd[(g + 1) & 1]);
                    else load(xn, r1n, r2n, 0, fa[0], pd[0]);            // first group of the next xi (after the last xi: harmless)
                    __builtin_amdgcn_sched_barrier(0);
                    const WFrag& oa = fa[g & 1];
                    const WPatch& o = pd[g & 1];
                    f32x2w v[NT][2];
#pragma unroll
                    for (int ct = 0; ct < NT; ++ct)
#pragma unroll
                        for (int e2 = 0; e2 < 2; ++e2) {
                            const f32x2w t1 = S1[nu] * o.d[ct][e2][0] + S2[nu] * o.d[ct][e2][1];
                            const f32x2w t2 = S1[nu] * o.d[ct][e2][2] + S2[nu] * o.d[ct][e2][3];
                            v[ct][e2] = t1 + sigma * t2;
                        }
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int rt = 0; rt < RTW; ++rt)
#pragma unroll
                            for (int ct = 0; ct < NT; ++ct)
                                M[ct][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4e(oa.a[rt], e), v[ct][e >> 1][e & 1], M[ct][rt], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                // Y[i][j] += A^T[i][xi] A^T[j][nu] M
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (AT[j][nu] != 0.f) {
                        const float k0 = c0 * AT[j][nu], k1 = c1 * AT[j][nu];
#pragma unroll
                        for (int ct = 0; ct < NT; ++ct)
#pragma unroll
                            for (int rt = 0; rt < RTW; ++rt) {
                                if constexpr (decltype(has0)::value) Y[ct][0][j][rt] += k0 * M[ct][rt];
                                if constexpr (decltype(has1)::value) Y[ct][1][j][rt] += k1 * M[ct][rt];
                            }
                    }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) { r1[ct] = r1n[ct]; r2[ct] = r2n[ct]; }
        };
        if constexpr (CF_WINO_PEEL == 2) {      // all four bodies (measured: see DESIGN)
            xi_body(0, std::true_type{}, std::false_type{});
            xi_body(1, std::true_type{}, std::true_type{});
            xi_body(2, std::true_type{}, std::true_type{});
            xi_body(3, std::false_type{}, std::true_type{});
        } else if constexpr (CF_WINO_PEEL) {
            xi_body(0, std::true_type{}, std::false_type{});
#pragma unroll 1
            for (int xi = 1; xi < 3; ++xi) xi_body(xi, std::true_type{}, std::true_type{});
            xi_body(3, std::false_type{}, std::true_type{});
        } else {
#pragma unroll 1
            for (int xi = 0; xi < 4; ++xi) xi_body(xi, std::true_type{}, std::true_type{});
        }
    }
    }       // per-position form
    __syncthreads();                 // every wave has finished reading h1
#pragma unroll
    for (int rt = 0; rt < RTW; ++rt) {
        const float4 b = *reinterpret_cast<const float4*>(wsl + G::OFF_B2 + (rt0 + rt) * 16 + 4 * lg);
#pragma unroll
        for (int ct = 0; ct < NT; ++ct)
#pragma unroll
            for (int i = 0; i < 2; ++i) {            // the two pixels (j = 0, 1) of an output row of the tile: one 8-byte store
                float* dst = kLaneTabW22<G> ? H1 + (rt0 + rt) * 16 * PIX + i * W + dsto
                                            : H1 + ((rt0 + rt) * 16 + 4 * lg) * PIX + smp[ct] * HW + (2 * ty[ct] + i) * W + 2 * tx[ct];
                const float bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    *reinterpret_cast<float2*>(dst + r * PIX) =
                        make_float2(cf_relu(Y[ct][i][0][rt][r] + bb[r]), cf_relu(Y[ct][i][1][rt][r] + bb[r]));
            }
    }
    if constexpr (RSPLIT > 1) __syncthreads();      // phase 3 reads all rows of this wave's own columns: both row halves in place
    else cf_wave_sync();
}

// ---- Winograd F(2x4, 3x3) form of the reflect-padded 3x3 on the 4x4 and 8x8 levels (phase 2 of PIPE == 6 geometries) ----
// F(2, 3) down the rows and F(4, 3) along the columns: per 2x4 output tile and channel pair 24 products instead of the 2 x 16 of
// two F(2x2) tiles, so the 3x3 runs 12 instead of 16 C^2 multiply-adds per pixel (a step 16 instead of 20):
//     Y = A2^T [ sum_ci U[ci] (.) (B2^T d[ci] B4) ] A4,     U = G2 w G4^T (packed once, fp64 -> fp32, k_step_pack),
// d = the 4x6 input patch of the tile (reflect-padded).  F(4, 3) is the Toom-Cook form on the points {0, 1, -1, 1/2, -1/2, inf}:
// every entry of B4^T ({0, +-1/4, +-1/2, +-1, -5/4}) and A4^T ({0, +-1, +-1/2, 1/4, +-1/8}) is exact in fp32, the 1/f_k of the
// construction (4, 2/3, -8/3) lives in the packed weights.  The integer points {0, +-1, +-2, inf} cost twice the error on the cifar10
// "extreme" fixture (9.2e-6 bits/dim against a 1e-5 bar); the half points keep F(2x2)'s 4.6e-6 (tests/test_winograd24.py).
// Mapping, 4x4: 8 samples x 2 tiles = the 16 lanes of ONE 16x16x4 column tile per workgroup; the four waves split the output ROWS
// (RTW = RT16 / 4 row tiles each) and each forms the Winograd-domain operands of all 16 tiles itself.  8x8 (4 samples): an image is
// 4 x 2 tiles, 2 samples fill a column tile, the workgroup has two; wave w takes column tile w & 1 and row half w >> 1 (RTW =
// RT16 / 2 = 2 as at 4x4: the same accumulators, the operands of a column tile are formed by two waves).  Per vertical index xi and
// group of 4 k-steps the lane sums its two patch rows once per patch column (A[c] = d[r1][c] + sigma d[r2][c], six values) and
// the six horizontal positions come from those with constant FMAs; the six position products accumulate in M[nu] over all k,
// and the output transform runs once per xi (Z = M A4, Y[i] += A2^T[i][xi] Z).
// h1 layout (written by phase 1 of the same geometry, w24_pix): 4x4: pixel (s, y, x) of row k sits at k PIX + 8 (4 y + ((x + y + k) & 3)) + s
// - the skew by y and by the channel parity puts the 32 lanes of a half wave (8 samples x 2 tile rows x 2 channels; the two tile rows
// share the patch row at a = 0 / 3) on distinct banks for every patch row and column.
// 8x8: a ds_read_b32 is served in two groups of 32 lanes on 32 banks; a group of a patch read is (2 channel parities) x (2 samples)
// x (4 tile rows) x (2 tile columns).  For a given patch element the four image rows have one parity and the two image columns are
// {1,3}, {0,4}, {1,5}, {2,6}, {3,7} or {4,6}: the same parity, and g = x2 ^ x1 (bits of x) tells the two apart in every pair.
// Word of pixel (s, y, x) inside row k (bits 7..0):
//     s1 | x1 | y0 ^ k1 | y2 y1 | s0 | g | x0 ^ k0
// - the low five bits (the bank) are distinct for the 32 lanes of a group for every patch element (lanes whose reflected row
// coincides read the same word), and the low six for all 64 lanes.  The word is a row part + a column part (w24_row / w24_col), so an operand address is one
// addition.  (tests/test_winograd24_8x8.py checks the order exhaustively.)
// 4x4, 16 samples per workgroup (Geo::ZSKIP): every output tile of a column tile has the same tile row, so a 32-lane group of a
// patch read is (16 samples) x (2 channel parities) at ONE pixel (y, x).  With R = 2 y + (x >> 1), the word of pixel (s, y, x)
// inside a row of parity k is
//     32 R + 16 ((x ^ k) & 1) + (s ^ 2 R)
// - a read group varies s and k at fixed (y, x): its banks 16 ((x ^ k) & 1) + (s ^ 2 R) are all 32;
// - a 32-lane group of phase 1's stores is two samples (s >> 1 fixed) x their 16 pixels at one k: bank bits 3..1 are
//   (s >> 1) ^ R, bit 0 is s & 1 and bit 4 is (x ^ k) & 1 - again all 32 (the order 16 (4 y + ((x + k) & 3)) + s puts those
//   stores on four banks).  (tests/test_w24_zero_skip.py checks both, and that the order is a bijection, exhaustively.)
__host__ __device__ constexpr int w24z_pix(int s, int y, int x, int kq) {
    const int R = 2 * y + (x >> 1);
    return 32 * R + 16 * ((x ^ kq) & 1) + ((s ^ (2 * R)) & 15);
}
template <class G> __host__ __device__ constexpr int w24_row(int s, int y, int kq) {
    return 128 * (s >> 1) + 32 * ((y ^ (kq >> 1)) & 1) + 8 * (y >> 1) + 4 * (s & 1);
}
template <class G> __host__ __device__ constexpr int w24_col(int x, int kq) {
    return 64 * ((x >> 1) & 1) + 2 * (((x >> 2) ^ (x >> 1)) & 1) + ((x ^ kq) & 1);
}
template <class G> __host__ __device__ constexpr int w24_pix(int s, int y, int x, int kq) {      // kq = row & 3
    if constexpr (G::ZSKIP) return w24z_pix(s, y, x, kq);
    else if constexpr (G::H == 4) return 8 * (4 * y + ((x + y + kq) & 3)) + s;
    else return w24_row<G>(s, y, kq) + w24_col<G>(x, kq);
}

// ---- per-lane address words of the F(2x4) form at 8x8, tabulated at compile time -------------------------------------------------
// Everything a lane needs to address the skewed h1 plane depends on (wave, lane) and the geometry alone; a step of the level kernel
// formed it afresh (twice: nothing may stay live across the 3x3).  w24_lane is the one definition of those words; kLaneTab holds
// them for the 256 threads of a workgroup, and a lane fetches its entry with 16-byte loads (five per step, L2 / L1 hits).
constexpr int cf_reflect(int v, int n) { return v < 0 ? -v : (v >= n ? 2 * (n - 1) - v : v); }      // padding_mode='reflect'
template <class G> struct alignas(16) W24Lane {
    int row[4];             // phase 2: BYTE offset of patch row a of this lane's output tile: 4 w24_row(smp, yrow[a], lg)
    int col[6];             // ... of patch column c, with the lane's k row of H1: 4 (HALF PIX + lg PIX + w24_col(xcol[c], lg))
    int dst;                // h2 epilogue: FLOAT offset of the tile's first pixel in row 4 lg of H1
    int pad;
    int pw[G::PTW][4];      // phase 1: skewed word of pixel pix[q] in a row with row & 3 = kq (float offset inside the row)
};
template <class G> __host__ __device__ constexpr W24Lane<G> w24_lane(int wave, int lane) {
    static_assert(kLaneTabW24<G>, "tabulated for the 8x8 level");
    constexpr int W = G::W, H = G::H, HW = G::HW, PIX = G::PIX, HALF = G::HALF, NCT = PIX / 128, TPS = HW / 8, TXN = W / 4;
    W24Lane<G> e{};
    const int l15 = lane & 15, lg = lane >> 4, li = lane & 31;
    const int tg = (wave % NCT) * 16 + l15;              // this lane's output tile (winograd24_phase2)
    const int smp = tg / TPS, ty = (tg % TPS) / TXN, tx = tg % TXN;
    for (int a = 0; a < 4; ++a) e.row[a] = 4 * w24_row<G>(smp, cf_reflect(2 * ty - 1 + a, H), lg);
    for (int c = 0; c < 6; ++c) e.col[c] = 4 * (HALF * PIX + lg * PIX + w24_col<G>(cf_reflect(4 * tx - 1 + c, W), lg));
    e.dst = 4 * lg * PIX + smp * HW + 2 * ty * W + 4 * tx;
    for (int q = 0; q < G::PTW; ++q) {
        const int pix = (wave * G::PTW + q) * 32 + li, pin = pix % HW;
        for (int kq = 0; kq < 4; ++kq) e.pw[q][kq] = w24_pix<G>(pix / HW, pin / W, pin % W, kq);
    }
    return e;
}
// the same for the F(2x2) form at 16x16, C = 16 (winograd_phase2 with one column tile per wave, phase 1 on 32-pixel tiles)
template <class G> struct alignas(16) W22Lane {
    int row[4];             // phase 2: rpart[a], BYTE offset of patch row a with the lane's k row of H1
    int col[4];             // ... cpart[a], byte offset of patch column a
    int pw[2];              // phase 1: parity-split word of pixel pix[q] in an even row (odd rows: ^ W / 2)
    int dst;                // h2 epilogue: FLOAT offset of the tile's first pixel in row 4 lg of H1
    int pad;
};
template <class G> __host__ __device__ constexpr W22Lane<G> w22_lane(int wave, int lane) {
    static_assert(G::PIPE == 3 && G::PTW == 2, "one column tile of 16 output tiles per wave");
    constexpr int W = G::W, H = G::H, HW = G::HW, PIX = G::PIX, HALF = G::HALF, TPS = HW / 4;
    W22Lane<G> e{};
    const int l15 = lane & 15, lg = lane >> 4, li = lane & 31;
    const int tg = wave * 16 + l15, ti = tg % TPS;       // this lane's output tile (winograd_phase2)
    const int smp = tg / TPS, ty = ti / (W / 2), tx = ti % (W / 2);
    for (int a = 0; a < 4; ++a) {
        const int yy = cf_reflect(2 * ty - 1 + a, H), xx = cf_reflect(2 * tx - 1 + a, W);
        e.row[a] = 4 * (HALF * PIX + lg * PIX + wino_pix<G>(smp * HW, yy, 0));
        e.col[a] = 4 * ((((xx ^ lg) & 1) * (W / 2)) + (xx >> 1));
    }
    for (int q = 0; q < 2; ++q) {
        const int pix = (wave * G::PTW + q) * 32 + li, pin = pix % HW;
        e.pw[q] = wino_pix<G>(pix - pin, pin / W, pin % W);
    }
    e.dst = 4 * lg * PIX + smp * HW + 2 * ty * W + 2 * tx;
    return e;
}
// F(2, 3) down the rows: B2^T row xi = d[r1] + sigma d[r2] over the four patch rows, sigma = -1 but at xi = 1.  w24_xi_is_zero:
// in an image of H rows, a tile of tile row ty gets +0 at xi from every patch: r1 and r2 are ONE image row under reflect padding
constexpr int w24_r1(int xi) { return xi == 0 ? 0 : (xi == 2 ? 2 : 1); }
constexpr int w24_r2(int xi) { return xi == 2 ? 1 : (xi == 3 ? 3 : 2); }
constexpr bool w24_xi_is_zero(int xi, int ty, int H) {
    return xi != 1 && cf_reflect(2 * ty - 1 + w24_r1(xi), H) == cf_reflect(2 * ty - 1 + w24_r2(xi), H);
}
template <class G> using LaneEntry = std::conditional_t<G::W24, W24Lane<G>, W22Lane<G>>;
template <class G> struct LaneTab { LaneEntry<G> e[kWaves * 64]; };
template <class G> constexpr LaneTab<G> make_lane_tab() {
    LaneTab<G> t{};
    for (int i = 0; i < kWaves * 64; ++i) {
        if constexpr (G::W24) t.e[i] = w24_lane<G>(i >> 6, i & 63);
        else t.e[i] = w22_lane<G>(i >> 6, i & 63);
    }
    return t;
}
template <class G> __device__ const LaneTab<G> kLaneTab = make_lane_tab<G>();
// the 16-byte word `i` of thread tid's entry
template <class G> __device__ __forceinline__ int4 lane_tab_word(int tid, int i) {
    return reinterpret_cast<const int4*>(&kLaneTab<G>.e[tid])[i];
}

// CF_W24_SPREAD (A/B builds of tools/dev/make_abl.py): 1 = the 8x8 level issues the patch reads of the next k-group one patch column
// per nu step, 0 = as one burst behind the vertical sums, as the 4x4 level does either way
#ifndef CF_W24_SPREAD
#define CF_W24_SPREAD 1
#endif
// tw (8x8): words 0 .. 2 of this thread's table entry (W24Lane), requested by the caller in front of the barrier that ends phase 1
template <class G>
__device__ __forceinline__ void winograd24_phase2(float* __restrict__ lds, const float* __restrict__ wsl, ws_rsrc_t rs, int lane,
                                                  int wave, const int4 (&tw)[3]) {
    constexpr int W = G::W, H = G::H, HW = G::HW, PIX = G::PIX, HALF = G::HALF, RT16 = G::RT16, KG4 = G::KG4;
    constexpr int NCT = PIX / 128;                       // column tiles (16 output tiles of 2x4 pixels) of the workgroup
    constexpr int RSP = G::WAVES / NCT;                  // waves that share a column tile and split the output rows
    static_assert(G::W24 && (NCT == 1 || NCT == 2) && RT16 % RSP == 0 && W % 4 == 0, "F(2x4, 3x3) geometry");
    // Zero skip (4x4, 16 samples, 8 waves): column tile ct holds the tiles of tile row ty = ct of all 16 samples, and the wave leaves
    // out the vertical index whose transform is d[r] - d[r] = +0 in every lane: xi = 0 at ty = 0, xi = 3 at ty = 1.  Its M would be
    // +0 (+0 gains +-0 per product of finite weights), its Z +0, and Y[0] = +0 + 1 (+0) resp. Y[1] += (-1)(+0) = -0 change no bit.
    constexpr bool ZS = G::ZSKIP;
    static_assert(!ZS || (NCT == 2 && HW / 8 == 2 && w24_xi_is_zero(0, 0, H) && w24_xi_is_zero(3, 1, H)),
                  "zero skip: the two patch rows of the skipped (xi, ty) must be ONE image row under the padding, and be subtracted");
    constexpr int RTW = RT16 / RSP;                      // 16-row tiles of this wave
    constexpr int NS = 6 * KG4;                         // (group, nu) steps per xi
    // nu order inside a group: 0 and 5 first, so that A0 / A5 die early and A1 .. A4 live on as P, Q, R, D
    constexpr int NU[6] = {0, 5, 1, 2, 3, 4};
    typedef float f32x2w __attribute__((ext_vector_type(2)));
    // 8x8 only: at 4x4 two of the six patch columns repeat another one's words, hipcc merges those reads inside a burst (32 values,
    // not 48), and the burst measured faster there
    constexpr bool SPREAD = CF_W24_SPREAD && H == 8;
    const int rt0 = __builtin_amdgcn_readfirstlane((NCT == 1 ? wave : wave / NCT) * RTW);
    float* H1 = lds + HALF * PIX;
    const int l15 = lane & 15, lg = lane >> 4;
    // 4x4 (derived: the table form measured slower there, profiles/lane_tables.md): this lane's output tile and its reflect-padded
    // patch rows; the patch columns are constants (one tile per image row).  The expressions are kept literally: hipcc's code for
    // that instantiation is then instruction for instruction what it was.
    const int ct = ZS ? __builtin_amdgcn_readfirstlane(wave % NCT) : 0;      // zero skip: this wave's column tile = its tile row
    const int smp = ZS ? l15 : l15 >> 1, ty = ZS ? ct : l15 & 1;
    int yrow[4];
    // 8x8: byte offsets of the patch rows and columns (the order is row part + column part) and the h2 offset, from the table
    int rpart[4], cpart[6], dsto = 0;
    if constexpr (H == 4) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int yy = 2 * ty - 1 + a;
            yrow[a] = yy < 0 ? -yy : (yy >= H ? 2 * (H - 1) - yy : yy);
        }
    } else {
        const int4 t0 = tw[0], t1 = tw[1], t2 = tw[2];
        rpart[0] = t0.x; rpart[1] = t0.y; rpart[2] = t0.z; rpart[3] = t0.w;
        cpart[0] = t1.x; cpart[1] = t1.y; cpart[2] = t1.z; cpart[3] = t1.w; cpart[4] = t2.x; cpart[5] = t2.y;
        dsto = t2.z;
    }
    f32x4 Y[2][4][RTW];
#pragma unroll
    for (int i = 0; i < (ZS ? 1 : 2); ++i)          // (zero skip: Y[1] behind the xi = 0 that half the waves run - not live across it)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int rt = 0; rt < RTW; ++rt) Y[i][j][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // operand addresses of one xi: patch rows r1 / r2 (B2^T row xi = d[r1] + sigma d[r2]) x the six patch columns
    // (BYTE offsets: an operand address is then this value + an immediate per k-step)
    auto addrs = [&](int xi, int (&o)[2][6]) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if constexpr (H == 4) {
                static_assert(w24_r1(0) == 0 && w24_r1(1) == 1 && w24_r1(2) == 2 && w24_r1(3) == 1 && w24_r2(0) == 2 && w24_r2(1) == 2 &&
                              w24_r2(2) == 1 && w24_r2(3) == 3, "the rows below are w24_r1 / w24_r2, which the zero-skip check reads");
                const int yy = h == 0 ? (xi == 0 ? yrow[0] : (xi == 2 ? yrow[2] : yrow[1]))
                                      : (xi == 2 ? yrow[1] : (xi == 3 ? yrow[3] : yrow[2]));
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    const int xx = c == 0 ? 1 : (c == 5 ? 2 : c - 1);
                    o[h][c] = 4 * (HALF * PIX + lg * PIX + w24_pix<G>(smp, yy, xx, lg & 1));
                }
            } else {
                const int rr = h == 0 ? (xi == 0 ? rpart[0] : (xi == 2 ? rpart[2] : rpart[1]))
                                      : (xi == 2 ? rpart[1] : (xi == 3 ? rpart[3] : rpart[2]));
#pragma unroll
                for (int c = 0; c < 6; ++c) o[h][c] = rr + cpart[c];
            }
        }
    };
    struct Raw { f32x2w d[2][6][2]; };                    // [row r1 / r2][patch column][k-step pair]
    struct WFrag { float4 a[RTW]; };
    // patch columns [c0, c1) of k-group kk (both patch rows, both k-step pairs: 8 values per column)
    auto load_raw_cols = [&](const int (&o)[2][6], int kk, Raw& r, int c0, int c1) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int c = c0; c < c1; ++c)
#pragma unroll
                for (int e2 = 0; e2 < 2; ++e2) {
                    const char* q0 = reinterpret_cast<const char*>(lds) + (16 * kk + 8 * e2) * PIX * 4;      // k-steps 4 kk + 2 e2 (+1)
                    const char* q1 = q0 + 4 * PIX * 4;
                    r.d[h][c][e2] = f32x2w{*reinterpret_cast<const float*>(q0 + o[h][c]), *reinterpret_cast<const float*>(q1 + o[h][c])};
                }
    };
    auto load_raw = [&](const int (&o)[2][6], int kk, Raw& r) { load_raw_cols(o, kk, r, 0, 6); };
    auto load_w = [&](int xi, int s, WFrag& f) {          // step s = kk * 6 + (index of nu in NU) of vertical index xi
        const int kk = s / 6, nu = NU[s % 6];
        const int fr = G::OFF_AW24 + (((xi * 6 + nu) * RT16 + rt0) * KG4 + kk) * 256;
#pragma unroll
        for (int rt = 0; rt < RTW; ++rt) f.a[rt] = ws_frag(rs, lane, fr + rt * KG4 * 256);
    };
    int o[2][6];
    // zero skip: a row of the 256-pixel planes is 1 KB, and the k rows of the upper half of the k-groups lie beyond what the offset
    // field of a ds_read2st64_b32 spans from the lane's address (255 x 256 B) - left to immediates, hipcc forms every such address
    // with a v_add_u32 of its own (470 per step).  The addresses move up ONCE per xi instead, by a value the compiler cannot fold
    int hoff = (KG4 / 2) * 16 * PIX * 4;
    if constexpr (ZS) asm volatile("" : "+s"(hoff));
    const int xi_first = ZS && ct == 0 ? 1 : 0;           // zero skip: the look-ahead chain starts at the wave's first xi
    addrs(xi_first, o);
    Raw raw;
    WFrag wf[2];                                          // weight fragments requested one step ahead
    load_raw(o, 0, raw);
    load_w(xi_first, 0, wf[0]);
    // A2^T[0][xi] = (1, 1, 1, 0), A2^T[1][xi] = (0, 1, -1, -1): xi = 0 and xi = 3 are peeled so that their zero half of the
    // output transform is not executed and, at xi = 0, Y[1] is not yet live (the loop keeps xi = 1, 2)
    // stop (zero skip only; wave-uniform): this xi is the wave's last, and nothing is requested for a next one
    auto xi_body = [&](const int xi, auto has0, auto has1, const bool stop) {
        const int xn = xi < 3 ? xi + 1 : 3;               // (after the last xi the prefetches re-read xi = 3: harmless)
        const float sigma = xi == 1 ? 1.f : -1.f;
        const float c0 = xi < 3 ? 1.f : 0.f, c1 = xi == 0 ? 0.f : (xi == 1 ? 1.f : -1.f);      // A2^T[0][xi], A2^T[1][xi]
        f32x4 M[6][RTW];
#pragma unroll
        for (int nu = 0; nu < 6; ++nu)
#pragma unroll
            for (int rt = 0; rt < RTW; ++rt) M[nu][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < KG4; ++kk) {
            f32x2w A[6][2];                               // vertical transform, once per patch column
#pragma unroll
            for (int c = 0; c < 6; ++c)
#pragma unroll
                for (int e2 = 0; e2 < 2; ++e2) A[c][e2] = raw.d[0][c][e2] + sigma * raw.d[1][c][e2];
            // the 48 patch values of the next k-group: as ONE burst here the reads fill the wave's LDS queue and hold its
            // instruction issue - MFMAs included - until they return; SPREAD: one patch column (8 values) goes out with each of
            // the six steps, into the same registers (raw is dead once A is formed)
            if (kk + 1 == KG4) addrs(xn, o);              // first group of the next xi: its operand addresses replace this xi's
            const int kn = kk + 1 < KG4 ? kk + 1 : 0;
            if constexpr (ZS) {
                if (kk + 1 == KG4 / 2) {                  // second half of the k-groups: the addresses move up by `hoff` (above)
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int c = 0; c < 6; ++c) o[h][c] += hoff;
                }
                if (kk + 1 < KG4 || !stop) load_raw(o, kn % (KG4 / 2), raw);
            } else if constexpr (!SPREAD) load_raw(o, kn, raw);
            // horizontal transform B4^T row nu:  nu 0: A0/4 - 5/4 A2 + A4;  1, 2: P +- Q (P = A4 - A2/4, Q = A3 - A1/4);
            // 3, 4: R +- (A3 - A1)/2 (R = A4 - A2);  5: A1/4 - 5/4 A3 + A5
            // (One lambda, called per step: written out inside the step loop, with the operand addresses of the next xi formed in
            // the burst's branch, the same arithmetic compiled to scalar halves - 4x4: 505 v_fma_f32 beside 263 v_pk_fma_f32,
            // now 31 beside 532, and 64 hazard s_nop instead of 216.  Why hipcc packs this form and not that one is not known.)
            auto operand = [&](const int nu, f32x2w (&v)[2]) {
#pragma unroll
                for (int e2 = 0; e2 < 2; ++e2) {
                    const f32x2w a0 = A[0][e2], a1 = A[1][e2], a2 = A[2][e2], a3 = A[3][e2], a4 = A[4][e2], a5 = A[5][e2];
                    if (nu == 0) v[e2] = 0.25f * a0 + (a4 - 1.25f * a2);
                    else if (nu == 1) v[e2] = (a4 - 0.25f * a2) + (a3 - 0.25f * a1);
                    else if (nu == 2) v[e2] = (a4 - 0.25f * a2) - (a3 - 0.25f * a1);
                    else if (nu == 3) v[e2] = (a4 - a2) + 0.5f * (a3 - a1);
                    else if (nu == 4) v[e2] = (a4 - a2) - 0.5f * (a3 - a1);
                    else v[e2] = 0.25f * a1 + (a5 - 1.25f * a3);
                }
            };
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                const int s = kk * 6 + t, nu = NU[t];
                if (s + 1 < NS) load_w(xi, s + 1, wf[(s + 1) & 1]);
                else if (!ZS || !stop) load_w(xn, 0, wf[0]);
                if constexpr (SPREAD) load_raw_cols(o, kn, raw, t, t + 1);
                __builtin_amdgcn_sched_barrier(0);
                f32x2w v[2];
                operand(nu, v);
                const WFrag& f = wf[s & 1];
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int rt = 0; rt < RTW; ++rt)
                        M[nu][rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4e(f.a[rt], e), v[e >> 1][e & 1], M[nu][rt], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // output transform of this xi: Z = M A4 (A4^T rows: 1 1 1 1 1 0 / 0 1 -1 1/2 -1/2 0 / 0 1 1 1/4 1/4 0 / 0 1 -1 1/8 -1/8 1),
        // Y[i] += A2^T[i][xi] Z
#pragma unroll
        for (int rt = 0; rt < RTW; ++rt) {
            const f32x4 s12 = M[1][rt] + M[2][rt], d12 = M[1][rt] - M[2][rt], s34 = M[3][rt] + M[4][rt], d34 = M[3][rt] - M[4][rt];
            const f32x4 Z[4] = {M[0][rt] + s12 + s34, d12 + 0.5f * d34, s12 + 0.25f * s34, d12 + 0.125f * d34 + M[5][rt]};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (decltype(has0)::value) Y[0][j][rt] += c0 * Z[j];
                if constexpr (decltype(has1)::value) Y[1][j][rt] += c1 * Z[j];
            }
        }
    };
    if (!ZS || ct == 1) xi_body(0, std::true_type{}, std::false_type{}, false);
    if constexpr (ZS) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int rt = 0; rt < RTW; ++rt) Y[1][j][rt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll 1
    for (int xi = 1; xi < 3; ++xi) xi_body(xi, std::true_type{}, std::true_type{}, ZS && ct == 1 && xi == 2);
    if (!ZS || ct == 0) xi_body(3, std::false_type{}, std::true_type{}, true);
    __syncthreads();                 // every wave has finished reading h1
#pragma unroll
    for (int rt = 0; rt < RTW; ++rt) {
        const float4 b = *reinterpret_cast<const float4*>(wsl + G::OFF_B2 + (rt0 + rt) * 16 + 4 * lg);
        const float bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {        // the four pixels of an output row of the tile: one 16-byte store
                float* dst = H == 4 ? H1 + ((rt0 + rt) * 16 + 4 * lg + r) * PIX + smp * HW + (2 * ty + i) * W
                                    : H1 + ((rt0 + rt) * 16 + r) * PIX + i * W + dsto;
                *reinterpret_cast<float4*>(dst) = make_float4(cf_relu(Y[i][0][rt][r] + bb[r]), cf_relu(Y[i][1][rt][r] + bb[r]),
                                                              cf_relu(Y[i][2][rt][r] + bb[r]), cf_relu(Y[i][3][rt][r] + bb[r]));
            }
    }
    __syncthreads();                 // phase 3 reads all rows of this wave's own columns: the other waves' row tiles in place
}

// ---- the conditioner: phases 1-3 of a step (shared by the forward and the inverse kernel) --------------
// In: Y0 = y0 plane (this wave's columns).  Out: acc3 = NN.4 output tiles (t rows / raw rows, packed-row
// layout of chan_of_row).  Uses the H region of LDS for h1 / h2; two workgroup barriers.
// CTX (specialist mode, coupling.py:39-47): 0 none; 1 per-sample bias sb[sample][C] added to the net OUTPUT
// (h = NN(x0) + CN(c), contextflow); 2 per-sample bias sb[sample][HID] added before the first ReLU (CN(c) concatenated
// to the net input = W[:, D:] CN(c) through the first 1x1).  soff[q] = this lane's row offset into sb.
// DUMP (training): the post-ReLU h1 / h2 planes go to the tape (16-byte stores of this wave's own columns).
// UPTO = 2: stop once h2 sits in LDS (k_flow_step_small runs the last 1x1 on 16x16x4 tiles itself; acc3 untouched).
template <class G, int CTX = 0, bool DUMP = false, int UPTO = 3>
__device__ __forceinline__ void conditioner_net(f32x16 (&acc3)[G::RT03][G::PTW], float* __restrict__ lds,
                                                const float* __restrict__ wsl, const int (&pix)[G::PTW],
                                                const int (&pin)[G::PTW], int lane, int tid, float* __restrict__ dbg,
                                                int64_t dbg_cols, int tile, const float* __restrict__ sb = nullptr,
                                                const int* soff = nullptr, StepTape tp = kNoTape, int B = 0) {
    constexpr int C = G::C, W = G::W, H = G::H, PIX = G::PIX, HALF = G::HALF, HID = G::HID;
    constexpr int PTW = G::PTW, RT03 = G::RT03, RT1 = G::RT1;
    float* Y0 = lds;
    float* H1 = lds + HALF * PIX;
    const int lk = lane >> 5;
    const ws_rsrc_t rs = ws_rsrc(wsl, G::WS_FLOATS);
    int4 tw2[3] = {};                // phase 2's words of this thread's kLaneTab entry, requested inside phase 1
    // ================= phase 1: h1 = relu(NN.0 y0 + b)                      (coupling.py:26)
    {
        f32x16 acc[RT1][PTW];
#pragma unroll
        for (int rt = 0; rt < RT1; ++rt)
#pragma unroll
            for (int q = 0; q < PTW; ++q) acc[rt][q] = bias_tile(wsl + G::OFF_B1 + rt * 32, lk);
        if constexpr (CTX == 2) {
#pragma unroll
            for (int rt = 0; rt < RT1; ++rt)
#pragma unroll
                for (int q = 0; q < PTW; ++q)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = rt * 32 + tile_row(r, lk);
                        if (row < HID) acc[rt][q][r] += sb[soff[q] + row];
                    }
        }
        // h1 goes to LDS in the pixel order phase 2 reads (F(2x4): skewed, w24_pix; F(2x2): parity-split, wino_pix).  Where the
        // geometry has a table (kLaneTab) the words of this lane's pixels come from there: phase 1's travel behind the MFMAs of
        // the dense phase, phase 2's behind the h1 stores and the barrier
        constexpr bool T24 = kLaneTabW24<G>, T22 = kLaneTabW22<G>;
        int4 w0{}, w1{};
        if constexpr (T24) { w0 = lane_tab_word<G>(tid, 3); w1 = lane_tab_word<G>(tid, 4); }
        else if constexpr (T22) w0 = lane_tab_word<G>(tid, 2);
        dense_phase<G, G::KS1, G::NG1, RT1>(acc, rs, G::OFF_A1, Y0, pix, lane);
        if constexpr (T24) {
#pragma unroll
            for (int i = 0; i < 3; ++i) tw2[i] = lane_tab_word<G>(tid, i);
        } else if constexpr (T22) {
            tw2[0] = lane_tab_word<G>(tid, 0); tw2[1] = lane_tab_word<G>(tid, 1); tw2[2] = w0;
        }
        // the parity-split h1 order of the Winograd form scatters a wave's pixels over its whole SAMPLE: where a sample spans
        // several waves (16x16), every wave must be done with its columns of what the H region held before (x / z plane)
        // (the F(2x4) order spreads every sample over the whole row)
        if constexpr (G::WINO && (G::HW > 32 * PTW || G::W24)) __syncthreads();
        const int tw1[2][4] = {{w0.x, w0.y, w0.z, w0.w}, {w1.x, w1.y, w1.z, w1.w}};
#pragma unroll
        for (int rt = 0; rt < RT1; ++rt)
#pragma unroll
            for (int q = 0; q < PTW; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = rt * 32 + tile_row(r, lk);
                    if constexpr (T24) {                // W24Lane::pw[q][row & 3]  (row & 3 = r & 3)
                        if (row < HID) H1[row * PIX + tw1[q][r & 3]] = cf_relu(acc[rt][q][r]);
                    } else if constexpr (T22) {         // W22Lane::pw[q], odd rows in the other column-parity block
                        if (row < HID) H1[row * PIX + (tw1[0][q] ^ ((r & 1) * (W / 2)))] = cf_relu(acc[rt][q][r]);
                    } else if constexpr (G::W24) {      // skewed pixel order of winograd24_phase2 (row & 3 = r & 3)
                        const int pw = w24_pix<G>((pix[q] - pin[q]) / G::HW, pin[q] / W, pin[q] % W, G::H == 4 ? r & 1 : r & 3);
                        if (row < HID) H1[row * PIX + pw] = cf_relu(acc[rt][q][r]);
                    } else if constexpr (G::WINO) {     // parity-split pixel order of winograd_phase2 (row & 1 = r & 1)
                        const int pw = wino_pix<G>(pix[q] - pin[q], pin[q] / W, pin[q] % W) ^ ((r & 1) * (W / 2));
                        if (row < HID) H1[row * PIX + pw] = cf_relu(acc[rt][q][r]);
                    } else {
                        if (row < HID) H1[row * PIX + pix[q]] = cf_relu(acc[rt][q][r]);
                    }
                }
        if constexpr (DUMP && G::WINO) {
            // the LDS plane is in the parity-split order: the tape's h1 (natural order, operand of the 3x3 weight gradient)
            // goes out from the accumulators, 128 contiguous bytes per row and half wave
#pragma unroll
            for (int q = 0; q < PTW; ++q) {
                const int b = tile * G::SPW + (pix[q] - pin[q]) / G::HW;
                if (b < B) {
                    float* dst = tp.h1 + (int64_t)b * HID * G::HW + pin[q];
#pragma unroll
                    for (int rt = 0; rt < RT1; ++rt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = rt * 32 + tile_row(r, lk);
                            if (row < HID) dst[row * G::HW] = cf_relu(acc[rt][q][r]);
                        }
                }
            }
            mask_store<G, RT1>(tp.m1, acc, tile, tid >> 6, lane);
        } else if constexpr (DUMP) {
            cf_wave_sync();
            rows_store_t<G, HID, HID>(tp.h1, H1, tile * G::SPW, B, tid >> 6, lane);
            mask_store<G, RT1>(tp.m1, acc, tile, tid >> 6, lane);
        }
    }
    __syncthreads();                 // h1 complete: the 3x3 taps read neighbouring waves' columns
    if (dbg) {
        float* d = dbg + (int64_t)C * dbg_cols;
        for (int e = tid; e < HID * PIX; e += G::NT) d[(int64_t)(e / PIX) * dbg_cols + (int64_t)tile * PIX + (e % PIX)] = H1[e];
    }

    // ================= phase 2: h2 = relu(NN.2 (*) h1 + b), 3x3, reflect padding   (coupling.py:27)
    if constexpr (G::WINO) {
        if constexpr (G::W24) {
            static_assert(!DUMP, "the F(2x4) form runs in the evaluation forward only");
            winograd24_phase2<G>(lds, wsl, rs, lane, tid >> 6, tw2);
        } else {
            winograd_phase2<G>(lds, wsl, rs, lane, tid >> 6, tw2);
        }
        if constexpr (DUMP) {            // h2 sits in LDS in natural order (own columns): plane store + mask words from the plane
            rows_store_t<G, HID, HID>(tp.h2, H1, tile * G::SPW, B, tid >> 6, lane);
#pragma unroll
            for (int rt = 0; rt < RT1; ++rt)
#pragma unroll
                for (int q = 0; q < PTW; ++q) {
                    unsigned bits = 0;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = rt * 32 + tile_row(r, lk);
                        if (row < HID) bits |= (H1[row * PIX + pix[q]] > 0.f ? 1u : 0u) << r;
                    }
                    tp.m2[((int64_t)(tile * G::NPT + (tid >> 6) * PTW + q) * RT1 + rt) * 64 + lane] = bits;
                }
        }
    } else {
        f32x16 acc[RT1][PTW];
#pragma unroll
        for (int rt = 0; rt < RT1; ++rt)
#pragma unroll
            for (int q = 0; q < PTW; ++q) acc[rt][q] = bias_tile(wsl + G::OFF_B2 + rt * 32, lk);
        // reflect-padded source pixel of a tap, as an index into lds[] (offsets, not pointers: a pointer array
        // loses the LDS address space and hipcc falls back to flat loads)
        auto tap_src = [&](int tap, int (&src)[PTW]) {
            const int dy = tap / 3 - 1, dx = tap % 3 - 1;              // wave-uniform
#pragma unroll
            for (int q = 0; q < PTW; ++q) {
                int yy = pin[q] / W + dy, xx = pin[q] % W + dx;
                yy = yy < 0 ? -yy : (yy >= H ? 2 * (H - 1) - yy : yy);       // reflect (padding_mode='reflect')
                xx = xx < 0 ? -xx : (xx >= W ? 2 * (W - 1) - xx : xx);
                src[q] = HALF * PIX + (pix[q] - pin[q]) + yy * W + xx + lk * PIX;
            }
        };
        if constexpr (G::PIPE == 2) {
            // every tap unrolled (compiler-scheduled inside).  The reflect-padded source offset of a tap splits into a row
            // part per (dy, pixel tile) and a column part per dx - the column inside the image row is the same for every
            // tile because W divides 32 - so the whole 3x3 costs 3 + 3 PTW reflections and one add per (tap, tile),
            // instead of a reflection pair per tap and tile inside the MFMA stream (27 VALU per tap at C = 16).
            static_assert(32 % W == 0, "a 32-pixel tile must hold whole image rows");
            int yo[3][PTW], xo[3];
            const int xin = pin[0] % W;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                int xx = xin + d - 1;
                xo[d] = xx < 0 ? -xx : (xx >= W ? 2 * (W - 1) - xx : xx);
#pragma unroll
                for (int q = 0; q < PTW; ++q) {
                    int yy = pin[q] / W + d - 1;
                    yy = yy < 0 ? -yy : (yy >= H ? 2 * (H - 1) - yy : yy);
                    yo[d][q] = HALF * PIX + (pix[q] - pin[q]) + yy * W + lk * PIX;
                }
            }
            float4 a_cur[RT1], a_nxt[RT1];
#pragma unroll
            for (int rt = 0; rt < RT1; ++rt) a_cur[rt] = ws_frag(rs, lane, G::OFF_A2 + rt * 256);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                int src[PTW];
#pragma unroll
                for (int q = 0; q < PTW; ++q) src[q] = yo[tap / 3][q] + xo[tap % 3];
#pragma unroll
                for (int cg = 0; cg < G::NCG; ++cg) {
                    const int g = tap * G::NCG + cg;
                    const int gn = g + 1 < G::NG2 ? g + 1 : G::NG2 - 1;
#pragma unroll
                    for (int rt = 0; rt < RT1; ++rt) a_nxt[rt] = ws_frag(rs, lane, G::OFF_A2 + (gn * RT1 + rt) * 256);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
#pragma unroll
                        for (int q = 0; q < PTW; ++q) {
                            const float bv = lds[src[q] + (8 * cg + 2 * e) * PIX];
#pragma unroll
                            for (int rt = 0; rt < RT1; ++rt)
                                acc[rt][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(f4e(a_cur[rt], e), bv, acc[rt][q], 0, 0, 0);
                        }
                    }
#pragma unroll
                    for (int rt = 0; rt < RT1; ++rt) a_cur[rt] = a_nxt[rt];
                }
            }
        } else if constexpr (G::PIPE == 0) {
            // compiler-scheduled form: one tap per loop trip, all NCG groups of the tap unrolled
            float4 a_cur[RT1], a_nxt[RT1];
#pragma unroll
            for (int rt = 0; rt < RT1; ++rt) a_cur[rt] = ws_frag(rs, lane, G::OFF_A2 + rt * 256);
#pragma unroll 1
            for (int tap = 0; tap < 9; ++tap) {
                int src[PTW];
                tap_src(tap, src);
#pragma unroll
                for (int cg = 0; cg < G::NCG; ++cg) {
                    const int g = tap * G::NCG + cg;
                    const int gn = min(g + 1, G::NG2 - 1);
#pragma unroll
                    for (int rt = 0; rt < RT1; ++rt)
                        a_nxt[rt] = G::ABL == 1 ? make_float4(0.5f, 0.25f, -0.5f, 0.125f + cg) : ws_frag(rs, lane, G::OFF_A2 + (gn * RT1 + rt) * 256);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
#pragma unroll
                        for (int q = 0; q < PTW; ++q) {
                            const float bv = G::ABL == 1 ? 0.001f * (src[q] + e) : lds[src[q] + (8 * cg + 2 * e) * PIX];
#pragma unroll
                            for (int rt = 0; rt < RT1; ++rt)
                                acc[rt][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(f4e(a_cur[rt], e), bv, acc[rt][q], 0, 0, 0);
                        }
                    }
#pragma unroll
                    for (int rt = 0; rt < RT1; ++rt) a_cur[rt] = a_nxt[rt];
                }
            }
        } else {
            // group g = tap*NCG + cg covers tap (dy,dx) and input channels 8cg .. 8cg+7.  The operands of group
            // g+1 are requested before the MFMAs of group g (two register sets, loads pinned by sched_barrier);
            // the source pixel of a tap is computed once per tap, one tap ahead.
            GroupOps<RT1, PTW> ops[2];
            auto load = [&](int fr, const int (&src)[PTW], int cg, GroupOps<RT1, PTW>& o) {   // fr: float offset of the group
                if constexpr (G::ABL == 1) {                      // timing ablation: operands from registers only
#pragma unroll
                    for (int rt = 0; rt < RT1; ++rt) o.a[rt] = make_float4(0.5f, 0.25f, -0.5f, 0.125f + cg);
#pragma unroll
                    for (int q = 0; q < PTW; ++q)
#pragma unroll
                        for (int e = 0; e < 4; ++e) o.b[e][q] = 0.001f * (src[q] + e);
                    return;
                }
#pragma unroll
                for (int rt = 0; rt < RT1; ++rt) o.a[rt] = ws_frag(rs, lane, fr + rt * 256);
#pragma unroll
                for (int q = 0; q < PTW; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e) o.b[e][q] = lds[src[q] + (8 * cg + 2 * e) * PIX];
            };
            int src_cur[PTW], src_nxt[PTW];
            tap_src(0, src_cur);
            load(G::OFF_A2, src_cur, 0, ops[0]);
#pragma unroll 1
            for (int tap = 0; tap < 9; ++tap) {
                tap_src(min(tap + 1, 8), src_nxt);
                const int fr = G::OFF_A2 + tap * G::NCG * RT1 * 256;
#pragma unroll
                for (int cg = 0; cg < G::NCG; ++cg) {                       // NCG is even: static ping-pong
                    const int fn = fr + (cg + 1) * RT1 * 256;               // fragments of the next group
                    if (cg + 1 < G::NCG) load(fn, src_cur, cg + 1, ops[(cg + 1) & 1]);
                    else load(tap < 8 ? fn : fr, src_nxt, 0, ops[0]);       // first group of the next tap
                    __builtin_amdgcn_sched_barrier(0);
                    group_mma<RT1, PTW>(acc, ops[cg & 1], 4);
                }
#pragma unroll
                for (int q = 0; q < PTW; ++q) src_cur[q] = src_nxt[q];
            }
        }
        __syncthreads();                 // every wave has finished reading h1 (taps cross pixel tiles)
#pragma unroll
        for (int rt = 0; rt < RT1; ++rt)
#pragma unroll
            for (int q = 0; q < PTW; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = rt * 32 + tile_row(r, lk);
                    if (row < HID) H1[row * PIX + pix[q]] = cf_relu(acc[rt][q][r]);
                }
        cf_wave_sync();              // h2 rows of all lanes in place (read below by other lanes of this wave)
        if constexpr (DUMP) {
            rows_store_t<G, HID, HID>(tp.h2, H1, tile * G::SPW, B, tid >> 6, lane);
            mask_store<G, RT1>(tp.m2, acc, tile, tid >> 6, lane);
        }
    }
    // no workgroup barrier: phase 3 reads only this wave's own pixel columns of h2
    if (dbg) {
        __syncthreads();
        float* d = dbg + (int64_t)(C + HID) * dbg_cols;
        for (int e = tid; e < HID * PIX; e += G::NT) d[(int64_t)(e / PIX) * dbg_cols + (int64_t)tile * PIX + (e % PIX)] = H1[e];
    }

    if constexpr (UPTO < 3) return;
    // ================= phase 3: h = NN.4 h2 + b ; affine map ; log-det        (coupling.py:28,52-66)
#pragma unroll
    for (int rt = 0; rt < RT03; ++rt)
#pragma unroll
        for (int q = 0; q < PTW; ++q) acc3[rt][q] = bias_tile(wsl + G::OFF_B3 + rt * 32, lk);
    if constexpr (CTX == 1) {
#pragma unroll
        for (int rt = 0; rt < RT03; ++rt)
#pragma unroll
            for (int q = 0; q < PTW; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ch = chan_of_row<G>(rt * 32 + (r & 3) + 8 * (r >> 2)) ;      // lk = 0 row; lk = 1 is +4
                    const int ch1 = chan_of_row<G>(rt * 32 + (r & 3) + 8 * (r >> 2) + 4);
                    const int c = lk ? ch1 : ch;
                    if ((lk ? ch1 : ch) >= 0) acc3[rt][q][r] += sb[soff[q] + c];
                }
    }
    dense_phase<G, G::KS3, G::NG3, RT03>(acc3, rs, G::OFF_A3, H1, pix, lane);
}

// ---- geometries ----------------------------------------------------------------------------------------
// Tile / loop form per shape, chosen by measurement on MI355X (tools/step_bench.py, B = 16384):
//   C16: 1 sample (256 px, 40 KB LDS, 3-4 workgroups/CU), compiler-scheduled tap loop    113 TFLOP/s
//   C32: 4 samples (256 px, 80 KB, 2/CU), explicit operand pipeline                        130 TFLOP/s
//   C64: 16 samples (256 px, 160 KB = the whole LDS, 1/CU), explicit pipeline, 4x2 tiles   136 TFLOP/s
// Which of them runs a step - per pass, shape, batch size and switch - is decided in ONE function, select() in cf_step_dispatch.h;
// the flop accounting (cf_flow_step_macs) reads the traits of the geometry that function names.  The backward has one geometry
// per shape (cf_step_bwd.h).
using G8 = Geo<8, 16, 16, 1, 0>;
using G16 = Geo<16, 16, 16, 1, 0>;
using G32 = Geo<32, 8, 8, 4, 1>;
using G64 = Geo<64, 4, 4, 16, 1>;
using G16s = Geo<16, 16, 16, 1, 2>;      // k_flow_step_small: 16x16x4 tiles for the 16-row phases, taps unrolled
using G8s = Geo<8, 16, 16, 1, 2>;
using G32v2 = Geo<32, 8, 8, 2, 1>;       // half the samples per workgroup: batches below one workgroup per CU
using G64v2 = Geo<64, 4, 4, 8, 1>;
using G8w = Geo<8, 16, 16, 1, 3>;
using G16w = Geo<16, 16, 16, 1, 3>;      // Winograd F(2x2,3x3) form of the 3x3 (winograd_phase2); 16x16: in k_flow_step_small
using G32w = Geo<32, 8, 8, 4, 3>;
using G64w2 = Geo<64, 4, 4, 8, 3>;       // 8 samples per workgroup, 2 workgroups / CU: two waves per column tile split the rows
using G64w24 = Geo<64, 4, 4, 8, 6>;      // ... in the Winograd F(2x4, 3x3) form (winograd24_phase2): the four waves split the rows
using G32w24 = Geo<32, 8, 8, 4, 6>;      // the 8x8 level in that form: two column tiles x two row halves
// the 4x4 level's F(2x4) form with 16 samples on 8 waves (512 threads, 160 KB: one workgroup / CU, two waves / SIMD as G64w24's two
// workgroups): a column tile holds ONE tile row, and its waves skip the vertical index that reflection zeroes (Geo::ZSKIP)
using G64z24 = Geo<64, 4, 4, 16, 6>;


int shape_id(int C, int H, int W) {
    if (C == 8 && H == 16 && W == 16) return 0;
    if (C == 16 && H == 16 && W == 16) return 1;
    if (C == 32 && H == 8 && W == 8) return 2;
    if (C == 64 && H == 4 && W == 4) return 3;
    return -1;
}

}  // namespace
