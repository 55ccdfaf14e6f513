// What every forward step kernel family shares: the design of the fused step, StepArgs, the weight packing (k_step_pack,
// launch_prepare), cf_lane_fresh and the WsChain record of the chained and level launches.  Included by the three family headers
// - cf_step_tile.h, cf_step_small.h, cf_step_rs.h - that cf_step.hip instantiates; everything lives in an anonymous namespace of
// the including translation unit.
#pragma once
#include "cf_step_common.h"

// One flow step — Conv1x1 -> ActNorm -> Coupling(1x1, ReLU, 3x3 reflect, ReLU, 1x1; affine map;
// log-det) — as ONE gfx950 kernel.  Reference: contextflow/model.py:129-147 (the per-step triple),
// layers/conv1x1.py:52-57, layers/actnorm.py:53-60, layers/coupling.py:26-29,52-66.
//
// Design (MI355X):
//  * every contraction runs on the exact-fp32 matrix cores (v_mfma_f32_32x32x2_f32): the weights
//    are the A operand (row = output channel), the activations the B operand (column = pixel), so
//    a result tile has the PIXEL on the lane and the CHANNELS in the 16 accumulator registers.
//    That makes every LDS access of the activation planes [channel][pixel] a run of 32 consecutive
//    floats per half-wave (bank-conflict free, also under the 3x3 tap shifts with reflection), and
//    puts t, log_s and x1 of one (channel, pixel) in the SAME lane for the affine epilogue;
//  * a workgroup (4 waves) owns PIX = 128/256 pixels = SPW whole samples; activations never leave
//    the CU between the five contractions: x -> [MFMA] y=W'x+b' (ActNorm folded into the 1x1
//    matrix) -> LDS -> h1 -> LDS -> 3x3 -> LDS -> h -> epilogue.  HBM traffic per step = read x once + write z once.
//    The 3x3 - 72 of the 80 C^2 HW multiply-adds of a step - is an implicit GEMM over the 9 taps in the direct-form
//    geometries, and Winograd F(2x2,3x3) on 16x16x4 tiles (16 of 36 products per output tile; cf_step_common.h:
//    winograd_phase2) in the PIPE = 3 geometries that cf_flow_step_fwd dispatches at benchmark batch sizes;
//  * weights are pre-packed per call by cf_flow_step_prepare into MFMA-fragment order (one 16-byte
//    load per lane = A fragments of 4 k-steps, 1 KiB per wave-instruction, L2-resident) and
//    software-prefetched one group ahead of the MFMAs that use them;
//  * log-det: lane-local sum over channels, shuffle-reduce over the lanes of one sample, one LDS
//    hop across waves, then a plain read-modify-write of ldj_acc[b] by the single owner of sample
//    b — no float atomics, bitwise reproducible.

namespace {

// host: the arguments of one forward-step launch, whichever kernel family runs it (sq: the step sits behind a Squeeze((2,2)),
// dbg: per-phase dumps of the test hook, sb: per-sample bias of the specialist coupling, tp: the training tape)
struct StepArgs {
    const float* x;
    float* z;
    float* ldj;
    const float* ws;
    int B;
    int64_t xbs;
    bool sq;
    hipStream_t s;
    float* dbg = nullptr;
    const float* sb = nullptr;
    StepTape tp = kNoTape;
};

// ---- weight packing (cf_flow_step_prepare) ---------------------------------------------------------
// A fragment of k-step s, row tile rt, lane l: A[row = rt*32 + (l&31)][k = 2s + (l>>5)]; 4 k-steps
// per float4: element ((g*RT + rt)*64 + l)*4 + e holds k-step 4g+e.
// blockIdx.y = flow step of a batch (cf_flow_step_prepare_batch: the steps of one resolution level pack side by side)
constexpr int kPrepBatch = 16;
struct StepPackBatch {
    const float *Wm[kPrepBatch], *t[kPrepBatch], *logs[kPrepBatch], *w1[kPrepBatch], *b1[kPrepBatch], *w2[kPrepBatch], *b2[kPrepBatch],
        *w3[kPrepBatch], *b3[kPrepBatch];
    float* ws[kPrepBatch];
    int w24;                             // also the F(2x4, 3x3) Winograd-domain weights of the 4x4 / 8x8 levels (not under CONTEXTFLOW_DIRECT_CONV=1)
};
template <class G>
__global__ __launch_bounds__(256) void k_step_pack(const StepPackBatch pb) {
    const int bi = blockIdx.y;
    const float* __restrict__ Wm = pb.Wm[bi]; const float* __restrict__ t = pb.t[bi]; const float* __restrict__ logs = pb.logs[bi];
    const float* __restrict__ w1 = pb.w1[bi]; const float* __restrict__ b1 = pb.b1[bi]; const float* __restrict__ w2 = pb.w2[bi];
    const float* __restrict__ b2 = pb.b2[bi]; const float* __restrict__ w3 = pb.w3[bi]; const float* __restrict__ b3 = pb.b3[bi];
    float* __restrict__ ws = pb.ws[bi];
    const int gtid = blockIdx.x * 256 + threadIdx.x, gsz = gridDim.x * 256;
    if (gtid == 0) {       // ldj_const = H*W*log|det Wm| + sum_c logs  (ws[1] holds log|det| from k_slogdet)
        float s = 0.f;
        for (int c = 0; c < G::C; ++c) s += logs[c];
        ws[0] = (float)G::HW * ws[1] + s;                    // conv1x1.py:53 + actnorm.py:58
    }
    for (int p = gtid; p < G::R03; p += gsz) {
        const int ch = chan_of_row<G>(p);
        ws[G::OFF_B0 + p] = ch >= 0 ? -t[ch] * expf(-logs[ch]) : 0.f;     // (x - t) e^{-logs} = e^{-logs} x - t e^{-logs}
        ws[G::OFF_B3 + p] = ch >= 0 ? b3[ch] : 0.f;
    }
    for (int p = gtid; p < G::R1; p += gsz) {
        ws[G::OFF_B1 + p] = p < G::HID ? b1[p] : 0.f;
        ws[G::OFF_B2 + p] = p < G::HID ? b2[p] : 0.f;
    }
    auto split = [](int e, int RT, int& g, int& rt, int& lane, int& j) {
        j = e & 3; lane = (e >> 2) & 63; const int q = e >> 8; rt = q % RT; g = q / RT;
    };
    int g, rt, lane, j;
    for (int e = gtid; e < G::NG0 * G::RT03 * 256; e += gsz) {            // phase 0: e^{-logs} Wm
        split(e, G::RT03, g, rt, lane, j);
        const int ch = chan_of_row<G>(rt * 32 + (lane & 31)), k = 2 * (4 * g + j) + (lane >> 5);
        ws[G::OFF_A0 + e] = (ch >= 0 && k < G::C) ? expf(-logs[ch]) * Wm[ch * G::C + k] : 0.f;
    }
    for (int e = gtid; e < G::NG1 * G::RT1 * 256; e += gsz) {             // phase 1: NN.0 (HID x HALF)
        split(e, G::RT1, g, rt, lane, j);
        const int row = rt * 32 + (lane & 31), k = 2 * (4 * g + j) + (lane >> 5);
        ws[G::OFF_A1 + e] = (row < G::HID && k < G::HALF) ? w1[row * G::HALF + k] : 0.f;
    }
    for (int e = gtid; e < G::NG2 * G::RT1 * 256; e += gsz) {             // phase 2: NN.2, k = tap*HID + ci
        split(e, G::RT1, g, rt, lane, j);
        const int row = rt * 32 + (lane & 31);
        const int tap = g / G::NCG, ci = 8 * (g % G::NCG) + 2 * j + (lane >> 5);
        ws[G::OFF_A2 + e] = (row < G::HID) ? w2[(row * G::HID + ci) * 9 + tap] : 0.f;
    }
    for (int e = gtid; e < G::NG3 * G::RT03 * 256; e += gsz) {            // phase 3: NN.4 (C x HID), packed rows
        split(e, G::RT03, g, rt, lane, j);
        const int ch = chan_of_row<G>(rt * 32 + (lane & 31)), k = 2 * (4 * g + j) + (lane >> 5);
        ws[G::OFF_A3 + e] = (ch >= 0 && k < G::HID) ? w3[ch * G::HID + k] : 0.f;
    }
    {   // Winograd-domain weights of NN.2: U[xi][nu] = G w G^T (fp64, rounded once), G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]]
        constexpr int HID = G::HID;
        const double Gm[4][3] = {{1, 0, 0}, {.5, .5, .5}, {.5, -.5, .5}, {0, 0, 1}};
        for (int e = gtid; e < 16 * HID * HID; e += gsz) {
            const int jj = e & 3, ln = (e >> 2) & 63, q = e >> 8;
            const int kg = q % G::KG4, rt16 = (q / G::KG4) % G::RT16, pos = q / (G::KG4 * G::RT16);
            const int co = rt16 * 16 + (ln & 15), ci = 4 * (4 * kg + jj) + (ln >> 4), xi = pos >> 2, nu = pos & 3;
            const float* wk = w2 + ((int64_t)co * HID + ci) * 9;
            double u = 0.0;
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) u += Gm[xi][a] * Gm[nu][b] * (double)wk[a * 3 + b];
            ws[G::OFF_AW + e] = (float)u;
        }
    }
    if (G::HAS_W24 && pb.w24) {
        // Winograd-domain weights of the F(2x4, 3x3) form (winograd24_phase2): U[xi][nu] = G2 w G4^T (fp64, rounded once), G2 as above,
        // G4 = the F(4, 3) Toom-Cook rows on the points {0, 1, -1, 1/2, -1/2, inf}
        constexpr int HID = G::HID;
        const double G2[4][3] = {{1, 0, 0}, {.5, .5, .5}, {.5, -.5, .5}, {0, 0, 1}};
        const double G4[6][3] = {{4, 0, 0}, {2. / 3, 2. / 3, 2. / 3}, {2. / 3, -2. / 3, 2. / 3}, {-8. / 3, -4. / 3, -2. / 3},
                                 {-8. / 3, 4. / 3, -2. / 3}, {0, 0, 1}};
        for (int e = gtid; e < 24 * HID * HID; e += gsz) {
            const int jj = e & 3, ln = (e >> 2) & 63, q = e >> 8;
            const int kg = q % G::KG4, rt16 = (q / G::KG4) % G::RT16, pos = q / (G::KG4 * G::RT16);
            const int co = rt16 * 16 + (ln & 15), ci = 4 * (4 * kg + jj) + (ln >> 4), xi = pos / 6, nu = pos % 6;
            const float* wk = w2 + ((int64_t)co * HID + ci) * 9;
            double u = 0.0;
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) u += G2[xi][a] * G4[nu][b] * (double)wk[a * 3 + b];
            ws[G::OFF_AW24 + e] = (float)u;
        }
    }
    if constexpr (G::RS16) {
        // k_flow_step_rs16: natural row order, element ((rt * NG + gi) * 64 + lane) * 4 + j = A[16 rt + (lane & 15)][4 (4 gi + j) + (lane >> 4)]
        constexpr int C = G::C, HID = G::HID, HALF = G::HALF;
        for (int p = gtid; p < C; p += gsz) { ws[G::OFF_RB0 + p] = -t[p] * expf(-logs[p]); ws[G::OFF_RB3 + p] = b3[p]; }
        for (int p = gtid; p < HID; p += gsz) { ws[G::OFF_RB1 + p] = b1[p]; ws[G::OFF_RB2 + p] = b2[p]; }
        auto split16 = [](int e, int NG, int& rt, int& gi, int& row, int& kk, int& j) {
            j = e & 3; const int ln = (e >> 2) & 63, q = e >> 8; gi = q % NG; rt = q / NG; row = 16 * rt + (ln & 15); kk = ln >> 4;
        };
        int rt, gi, row, kk, j;
        for (int e = gtid; e < (C / 16) * (C / 16) * 256; e += gsz) {                     // e^{-logs} Wm
            split16(e, C / 16, rt, gi, row, kk, j);
            const int k = 4 * (4 * gi + j) + kk;
            ws[G::OFF_RA0 + e] = expf(-logs[row]) * Wm[row * C + k];
        }
        for (int e = gtid; e < (HID / 16) * (HALF / 16) * 256; e += gsz) {                // NN.0
            split16(e, HALF / 16, rt, gi, row, kk, j);
            ws[G::OFF_RA1 + e] = w1[row * HALF + 4 * (4 * gi + j) + kk];
        }
        for (int e = gtid; e < (HID / 16) * 9 * (HID / 16) * 256; e += gsz) {             // NN.2: group = tap * (HID / 16) + channel group
            split16(e, 9 * (HID / 16), rt, gi, row, kk, j);
            const int tap = gi / (HID / 16), ci = 4 * (4 * (gi % (HID / 16)) + j) + kk;
            ws[G::OFF_RA2 + e] = w2[(row * HID + ci) * 9 + tap];
        }
        for (int e = gtid; e < (C / 16) * (HID / 16) * 256; e += gsz) {                   // NN.4
            split16(e, HID / 16, rt, gi, row, kk, j);
            ws[G::OFF_RA3 + e] = w3[row * HID + 4 * (4 * gi + j) + kk];
        }
    }
    if constexpr (G::SMALL) {
        // operands of the 16x16x4 phases: A fragment of k-step s, lane l = A[row = l & 15][k = 4 s + (l >> 4)];
        // element e = (group * 64 + lane) * 4 + j holds k-step 4 group + j
        for (int p = gtid; p < 16; p += gsz) {
            const int ch = chan_of_row16<G>(p);
            ws[G::OFF_SB0 + p] = ch >= 0 ? -t[ch] * expf(-logs[ch]) : 0.f;
            ws[G::OFF_SB3 + p] = ch >= 0 ? b3[ch] : 0.f;
        }
        for (int e = gtid; e < G::SG0 * 256; e += gsz) {
            const int jj = e & 3, ln = (e >> 2) & 63, gg = e >> 8, ch = chan_of_row16<G>(ln & 15), k = 4 * (4 * gg + jj) + (ln >> 4);
            ws[G::OFF_SA0 + e] = (ch >= 0 && k < G::C) ? expf(-logs[ch]) * Wm[ch * G::C + k] : 0.f;
        }
        for (int e = gtid; e < G::SG3 * 256; e += gsz) {
            const int jj = e & 3, ln = (e >> 2) & 63, gg = e >> 8, ch = chan_of_row16<G>(ln & 15), k = 4 * (4 * gg + jj) + (ln >> 4);
            ws[G::OFF_SA3 + e] = (ch >= 0 && k < G::HID) ? w3[ch * G::HID + k] : 0.f;
        }
        if constexpr (G::HID16) {
            for (int e = gtid; e < G::SG1 * 256; e += gsz) {               // NN.0: 16 rows x HALF
                const int jj = e & 3, ln = (e >> 2) & 63, gg = e >> 8, row = ln & 15, k = 4 * (4 * gg + jj) + (ln >> 4);
                ws[G::OFF_SA1 + e] = k < G::HALF ? w1[row * G::HALF + k] : 0.f;
            }
            for (int e = gtid; e < 9 * 256; e += gsz) {                    // NN.2: group = tap, k = input channel
                const int jj = e & 3, ln = (e >> 2) & 63, tap = e >> 8, row = ln & 15, ci = 4 * jj + (ln >> 4);
                ws[G::OFF_SA2 + e] = w2[(row * G::HID + ci) * 9 + tap];
            }
        }
    }
}

// Level kernels: this lane's index inside its wave, formed afresh where it is called (an asm statement with no inputs is neither
// hoisted nor merged).  With the wave's index in a scalar register, a step of a level kernel rebuilds its thread index - and every
// address table derived from it - per step, and the level loop carries no vector register at all: left to threadIdx.x, hipcc
// hoists those tables in front of the loop and keeps them live across every phase (74 - 82 spilled registers).
__device__ __forceinline__ int cf_lane_fresh() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}
// Chained / level launches: the packed tables of the n <= kChain consecutive steps of one resolution level, by value in the kernel
// arguments
constexpr int kChain = 4;
struct WsChain { const float* ws[kChain]; };

extern "C" int cf_slogdet_inverse_batch(int n, const float* const* Wm, int C, float* const* logabsdet, float* const* inv, cf_stream_t stream);

// n <= kPrepBatch steps of one shape: ONE factorisation launch (log|det Wm| into ws[1]; winv: also Wm^-1, training) and ONE
// packing launch
template <class G>
int launch_prepare(const StepPackBatch& pb, int n, float* const* winv, hipStream_t s) {
    float* lad[kPrepBatch];
    for (int i = 0; i < n; ++i) lad[i] = pb.ws[i] + 1;
    int rc = cf_slogdet_inverse_batch(n, pb.Wm, G::C, lad, winv, (cf_stream_t)s);
    if (rc) return rc;
    int blocks = (G::WS_FLOATS + 255) / 256;
    if (blocks > 512) blocks = 512;
    k_step_pack<G><<<dim3(blocks, n), dim3(256), 0, s>>>(pb);
    return 0;
}

}  // namespace
