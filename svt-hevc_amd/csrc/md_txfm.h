/* md_txfm.h - the transform leaves of the mode-decision kernels (md_kernels.hip): the 16x16 and 32x32 forward transforms of the full loops on the matrix cores, one
 * transform unit of ProductFullLoop (EbFullLoop.c:185-446) / FullLoop_R + CuFullDistortionFastTuMode_R (:579-1066), PerformInverseTransformRecon of the winner
 * (Codec/EbProductCodingLoop.c:1334-1414), the luma full loop of a unit's candidate and TuCalcCostLuma (Codec/EbRateDistortionCost.c:289-375). */
#pragma once
#include "encdec_device.h"
#include "md_logic.h"
#include "md_state.h"
#include "md_intra.h"

/* ---- the 16x16 and 32x32 forward transforms of the full loops on the MATRIX CORES (round 6) ----------------------------------------------------------------------------
 * Transform16x16 / Transform32x32Estimate (C_DEFAULT/EbTransforms_C.c: two partial-butterfly passes) are exact integer evaluations of C . X . C^T with a rounding shift
 * after each pass (txfm_mfma.hip; the Estimate forms wrap the first butterfly levels to 16 bits, which no sum reaches while the pass's inputs stay below 2^14 (16x16) /
 * 2^13 (32x32): checked per unit, the register butterflies take the unit otherwise - never on 8-bit video, where |T1| <= 16 . 90 . 255 >> 4).  Here the products run as
 * v_mfma_f32_16x16x16_f16 / v_mfma_f32_32x32x8_f16 ON EXACT INTEGERS: residuals (|x| <= 255) and matrix entries (|c| <= 90) are f16 values, their sums of 16 / 32
 * products stay below 2^24 (exact in the f32 accumulator); the 16-bit intermediate of pass 2 goes in as two exact planes T1 = 64 H + L (|H| <= 512, 0 <= L < 64).
 * Why, on a path that is not FLOP-bound: the unit chain is bound by INSTRUCTIONS ISSUED PER WAVE.  The butterflies keep a row per lane - N lanes of 64 busy, ~560 issue
 * slots for a 16x16 unit and ~800 for its quantiser; the matrix form keeps all 64 lanes busy (4 / 16 coefficients a lane, already where the quantiser wants them) in ~150.
 * Pass 1 is computed transposed (T1^T = S . C^T) so that a lane's accumulator registers ARE its B operand of pass 2 (out = C . T1^T): no transpose, no LDS.
 * The constant operand C (lane l: C_N[l % N][its K slots]) is the same for both passes; a workgroup keeps it in LDS (s_dct_op), filled once per launch. */
typedef _Float16 md_v4h __attribute__((ext_vector_type(4)));
typedef float md_v4f __attribute__((ext_vector_type(4)));
typedef float md_v16f __attribute__((ext_vector_type(16)));
static __shared__ int s_md_force_bfly;       /* debug (MdPictureDev.force_butterflies), set once per launch beside the operands below */
static __shared__ uint32_t s_dct_op[12][64]; /* [0..1]: 16x16, [2 + 2 s .. 3 + 2 s]: 32x32 K-slice s, [10..11]: two 8x8 matrices on the diagonal of a 16x16 one; two dwords = four f16 */
__device__ __forceinline__ void md_dct_operands_init(int force_butterflies)
{
    const int t = threadIdx.x;
    if (t == 64)
        s_md_force_bfly = force_butterflies;
    if (t < 64) {
        union { md_v4h h; uint32_t w[2]; } u;
        for (int i = 0; i < 4; i++)
            u.h[i] = (_Float16)(float)d_T32[2 * (t & 15)][4 * (t >> 4) + i];
        s_dct_op[0][t] = u.w[0], s_dct_op[1][t] = u.w[1];
        for (int i = 0; i < 4; i++) { /* diag(C8, C8): the chroma pair of a 16x16 unit as ONE 16x16 product (md_chroma_pair8) */
            const int r = t & 15, k = 4 * (t >> 4) + i;
            u.h[i] = (_Float16)(float)((r >> 3) == (k >> 3) ? d_T32[4 * (r & 7)][k & 7] : 0);
        }
        s_dct_op[10][t] = u.w[0], s_dct_op[11][t] = u.w[1];
        for (int sl = 0; sl < 4; sl++) {
            for (int i = 0; i < 4; i++)
                u.h[i] = (_Float16)(float)d_T32[t & 31][8 * sl + 4 * (t >> 5) + i];
            s_dct_op[2 + 2 * sl][t] = u.w[0], s_dct_op[3 + 2 * sl][t] = u.w[1];
        }
    }
}
__device__ __forceinline__ md_v4h md_h4(int a, int b, int c, int d)
{
    md_v4h r;
    r[0] = (_Float16)(short)a, r[1] = (_Float16)(short)b, r[2] = (_Float16)(short)c, r[3] = (_Float16)(short)d; /* v_cvt_f16_i16: |values| <= 512, exact */
    return r;
}
__device__ __forceinline__ md_v4h md_dct_op(int slot, int lane)
{
    union { md_v4h h; uint32_t w[2]; } u;
    u.w[0] = s_dct_op[slot][lane], u.w[1] = s_dct_op[slot + 1][lane];
    return u.h;
}
/* coefficients of the N x N unit (N = 16: 4 per lane, coefficient (4 (lane >> 4) + i, lane & 15); N = 32: 16 per lane, coefficient (mfma row(v, lane >> 5), lane & 31)) ->
 * out[]; returns false (in every lane) when the unit leaves the wrap-free domain of the Estimate butterflies */
template <int N>
__device__ __forceinline__ bool md_fwd_mfma(int lane, const uint8_t *src, int srcPitch, const uint8_t *pred, int predPitch, int fs1, int fs2, int (&out)[N * N / 64])
{
    const int off1 = 1 << (fs1 - 1), off2 = 1 << (fs2 - 1);
    if constexpr (N == 16) {
        const int j = lane & 15, g = lane >> 4;
        const uint32_t a = *reinterpret_cast<const uint32_t *>(src + j * srcPitch + 4 * g), b = *reinterpret_cast<const uint32_t *>(pred + j * predPitch + 4 * g);
        const md_v4h A = md_h4((int)(a & 0xFF) - (int)(b & 0xFF), (int)((a >> 8) & 0xFF) - (int)((b >> 8) & 0xFF), (int)((a >> 16) & 0xFF) - (int)((b >> 16) & 0xFF),
                               (int)(a >> 24) - (int)(b >> 24));
        const md_v4h C = md_dct_op(0, lane);
        const md_v4f z = {0.f, 0.f, 0.f, 0.f};
        const md_v4f t1 = __builtin_amdgcn_mfma_f32_16x16x16f16(A, C, z, 0, 0, 0); /* T1^T[4 g + i][lane & 15] */
        int t[4];
        bool wide = false;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            t[i] = (int)(int16_t)(((int)t1[i] + off1) >> fs1);
            wide = wide || t[i] > 16383 || t[i] < -16383;
        }
        if (__ballot(wide))
            return false;
        const md_v4h H = md_h4(t[0] >> 6, t[1] >> 6, t[2] >> 6, t[3] >> 6), Lo = md_h4(t[0] & 63, t[1] & 63, t[2] & 63, t[3] & 63);
        const md_v4f dh = __builtin_amdgcn_mfma_f32_16x16x16f16(C, H, z, 0, 0, 0), dl = __builtin_amdgcn_mfma_f32_16x16x16f16(C, Lo, z, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; i++)
            out[i] = (int)(int16_t)((((int)dh[i] << 6) + (int)dl[i] + off2) >> fs2);
        return true;
    } else {
        static_assert(N == 32, "matrix-core forms: 16x16 and 32x32");
        const int m = lane & 31, h = lane >> 5;
        md_v16f acc;
#pragma unroll
        for (int v = 0; v < 16; v++)
            acc[v] = 0.f;
        md_v4h C[4];
#pragma unroll
        for (int sl = 0; sl < 4; sl++) {
            const uint32_t a = *reinterpret_cast<const uint32_t *>(src + m * srcPitch + 8 * sl + 4 * h), b = *reinterpret_cast<const uint32_t *>(pred + m * predPitch + 8 * sl + 4 * h);
            const md_v4h A = md_h4((int)(a & 0xFF) - (int)(b & 0xFF), (int)((a >> 8) & 0xFF) - (int)((b >> 8) & 0xFF), (int)((a >> 16) & 0xFF) - (int)((b >> 16) & 0xFF),
                                   (int)(a >> 24) - (int)(b >> 24));
            C[sl] = md_dct_op(2 + 2 * sl, lane);
            acc = __builtin_amdgcn_mfma_f32_32x32x8f16(A, C[sl], acc, 0, 0, 0);
        }
        int t[16];
        bool wide = false;
#pragma unroll
        for (int v = 0; v < 16; v++) { /* T1^T[row(v, h)][m] */
            t[v] = (int)(int16_t)(((int)acc[v] + off1) >> fs1);
            wide = wide || t[v] > 8191 || t[v] < -8191;
        }
        if (__ballot(wide))
            return false;
        md_v16f dh, dl;
#pragma unroll
        for (int v = 0; v < 16; v++)
            dh[v] = 0.f, dl[v] = 0.f;
#pragma unroll
        for (int sl = 0; sl < 4; sl++) { /* the accumulator registers 4 sl .. 4 sl + 3 hold exactly K-slice sl of pass 2 */
            const md_v4h H = md_h4(t[4 * sl] >> 6, t[4 * sl + 1] >> 6, t[4 * sl + 2] >> 6, t[4 * sl + 3] >> 6);
            const md_v4h Lo = md_h4(t[4 * sl] & 63, t[4 * sl + 1] & 63, t[4 * sl + 2] & 63, t[4 * sl + 3] & 63);
            dh = __builtin_amdgcn_mfma_f32_32x32x8f16(C[sl], H, dh, 0, 0, 0);
            dl = __builtin_amdgcn_mfma_f32_32x32x8f16(C[sl], Lo, dl, 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 16; v++)
            out[v] = (int)(int16_t)((((int)dh[v] << 6) + (int)dl[v] + off2) >> fs2);
        return true;
    }
}

/* the coefficient-bit estimator (rate_device.h) as ONE function for every transform size: inlined into the four sizes of md_full_loop_unit it was 2.5 K instructions four
 * times over in a kernel whose unit loop does not fit the instruction cache (SQC_TC_INST_REQ: ~760 instruction lines from L2 per unit, profiles/r06_j) */
__device__ __noinline__ uint32_t md_coeff_bits(const SvtAmdCabacCost *cost, const int16_t *qbuf, int N, int lga, uint32_t nz, int type, int intra_mode, int component, int lane, int S4,
                                               const RateTables *rt)
{
    MD_LDS(cost), MD_LDS(qbuf), MD_LDS(rt);
    const SvtAmdTuInfo ti = {nz, (uint8_t)type, (uint8_t)intra_mode, 4 /* EB_INTRA_CHROMA_DM */, (uint8_t)component};
    return coeff_bits_lanes(*cost, qbuf, (uint32_t)N, lga, ti, lane < S4, lane, lane & (S4 - 1), *rt);
}

/* One transform unit of ProductFullLoop (EbFullLoop.c:185-446) / FullLoop_R + CuFullDistortionFastTuMode_R (:579-1066) on lanes r = 0..N-1 of
 * the calling wave: residual -> EstimateTransform -> quantiser -> coefficient-domain distortion -> coefficient bits.  src / pred: the unit's
 * source and prediction (pitches in samples); recon_coeff: the de-quantised coefficients (N x N, pitch N) for PerformInverseTransformRecon, or
 * null; pf: partial-frequency mode (1 = N2: only the low (N/2)^2 coefficients are quantised, measured and priced); type / component: of the
 * candidate and the plane (rate tables).  Returns (every lane) the unit's sums. */
template <int N>
__device__ MD_LEAF_CALL MdFl md_full_loop_unit(int lane, const uint8_t *src, int srcPitch, const uint8_t *pred, int predPitch, int16_t *recon_coeff, int16_t *tile,
                                                  int16_t *qbuf, int qp, int slice_type, const SvtAmdCabacCost &cost, int type, int intra_mode, int component, int pf, const RateTables &rt)
{
    constexpr int LG = N == 32 ? 5 : N == 16 ? 4 : N == 8 ? 3 : 2;
    constexpr int fs1 = N == 32 ? 6 : N == 16 ? 4 : N == 8 ? 2 : 1, fs2 = N == 4 ? 8 : 9, wrap = N == 32 ? 2 : N == 16 ? 1 : 0;
    MD_LDS(src), MD_LDS(pred), MD_LDS(tile), MD_LDS(qbuf), MD_LDS(&cost), MD_LDS(&rt);
    if (recon_coeff)
        MD_LDS(recon_coeff);
    MD_TR(50);
    const int qpRem = qp % 6, qpPer = qp / 6;
    const uint32_t QF = qpRem == 0 ? 26214u : qpRem == 1 ? 23302u : qpRem == 2 ? 20560u : qpRem == 3 ? 18396u : qpRem == 4 ? 16384u : 14564u;
    const int FFv = qpRem == 0 ? 40 : qpRem == 1 ? 45 : qpRem == 2 ? 51 : qpRem == 3 ? 57 : qpRem == 4 ? 64 : 72;
    const int tshift = 7 - LG, shiftedQBits = 14 + qpPer + tshift;
    const uint32_t offs = ((slice_type == 2 || slice_type == 3) ? 171u : 85u) << (shiftedQBits - 9);
    const int shiftedFFunc = qpPer > 8 ? FFv << (qpPer - 2) : FFv << qpPer;
    const int shiftNum = qpPer > 8 ? 20 - 14 - tshift - 2 : 20 - 14 - tshift, iq_offset = 1 << (shiftNum - 1);
    const int area = N >> pf;
    unsigned nz = 0, d0 = 0, d1 = 0;
    auto quantise = [&](int v, bool inside, int &q, int &c) {
        /* the products of the quantiser fit 24 x 24 bits (coefficients are 16-bit values, the scaling factors below 2^15): v_mul_i32_i24 is a full-rate instruction,
         * v_mul_lo_u32 a quarter-rate one */
        const int sign = v < 0 ? -1 : 1;
        int tq = abs(v);
        tq = (int)__umul24((uint32_t)tq, QF);
        tq = (int)((uint32_t)tq + offs);
        tq >>= shiftedQBits;
        q = clip16i(sign * tq);
        c = clip16i((__mul24(q, shiftedFFunc) + iq_offset) >> shiftNum);
        if (inside) {
            const int df = (int16_t)(v - c);
            nz += q != 0, d0 += (uint32_t)__mul24(df, df), d1 += (uint32_t)__mul24(v, v);
        }
    };
    bool on_matrix_cores = false;
    if constexpr (N == 16 || N == 32) {
        int co[N * N / 64];
        on_matrix_cores = !s_md_force_bfly && md_fwd_mfma<N>(lane, src, srcPitch, pred, predPitch, fs1, fs2, co); /* wave-uniform */
        if (on_matrix_cores) {
            MD_TR(52);
            const int k = lane & (N - 1);
            /* the quantiser without a branch per coefficient (a lane's coefficients lie inside or outside the quantised area one by one: each test was an exec-mask
             * region of its own): a coefficient outside contributes zeros to the sums and lands in a word of the buffer nobody reads */
            const bool col_in = k < area;
#pragma unroll
            for (int i = 0; i < N * N / 64; i++) {
                const int k2 = N == 16 ? 4 * (lane >> 4) + i : (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5); /* the accumulator's row */
                const bool inside = col_in && k2 < area;
                const int v = inside ? co[i] : 0;
                int tq = abs(v);
                tq = (int)__umul24((uint32_t)tq, QF);
                tq = (int)((uint32_t)tq + offs);
                tq >>= shiftedQBits;
                const int q = v < 0 ? -tq : tq; /* |q| <= 2^14: no clip */
                const int c = clip16i((__mul24(q, shiftedFFunc) + iq_offset) >> shiftNum);
                const int df = (int16_t)(v - c);
                nz += q != 0, d0 += (uint32_t)__mul24(df, df), d1 += (uint32_t)__mul24(v, v);
                qbuf[k2 * N + k] = (int16_t)q; /* (outside the area: zero, never read) */
                if (recon_coeff && inside)
                    recon_coeff[k2 * N + k] = (int16_t)c;
            }
        }
    }
    if (__builtin_expect(!on_matrix_cores, N < 16)) { /* (16x16 / 32x32: the fall-back of a unit outside the matrix form's domain - out of the way of the hot path's instruction stream) */
    const int r = lane & (N - 1);
    const bool active = lane < N;
    int x[N];
    if (active) { /* rows start on word boundaries (units sit on 4-sample grids of word-aligned planes) */
        const uint32_t *sw = reinterpret_cast<const uint32_t *>(src + r * srcPitch), *pw = reinterpret_cast<const uint32_t *>(pred + r * predPitch);
#pragma unroll
        for (int j = 0; j < N; j += 4) {
            const uint32_t a = sw[j >> 2], b = pw[j >> 2];
#pragma unroll
            for (int k = 0; k < 4; k++)
                x[j + k] = (int)((a >> (8 * k)) & 0xFFu) - (int)((b >> (8 * k)) & 0xFFu);
        }
    } else {
#pragma unroll
        for (int j = 0; j < N; j++)
            x[j] = 0;
    }
    MD_TR(51);
    /* the transform on the unit's N row-lanes (pass 1, transpose through LDS, pass 2), its coefficients straight into the quantiser's buffer (row-major, 16-bit: what the
     * second pass produces) - and the QUANTISER ON ALL 64 LANES: a lane owns N*N/64 consecutive coefficients (16 / 4 / 1 of a 32x32 / 16x16 / 8x8 unit) instead of a whole
     * column on N lanes: a 16x16 unit's quantiser is 4 coefficients deep per lane, not 16 (the unit chain is bound by instructions issued per wave). */
    {
        constexpr int P = TxRegTile<N>::PITCH;
        int16_t *t_ = tile; /* ONE unit per call, on lanes 0..N-1; the other lanes run along on zeros and leave no trace */
        fwd_1d_regs<N>(x, fs1, wrap, [&](int k, int16_t v) {
            if (active)
                t_[k * P + r] = v;
        });
        EP_WAVE_SYNC();
#pragma unroll
        for (int j = 0; j < N; j += 2) {
            const uint32_t w = *(const uint32_t *)&t_[r * P + j];
            x[j] = (int16_t)(w & 0xffffu), x[j + 1] = (int16_t)(w >> 16);
        }
        fwd_1d_regs<N>(x, fs2, wrap, [&](int k, int16_t v) {
            if (active)
                qbuf[k * N + r] = v; /* coefficient (k, r) */
        });
        EP_WAVE_SYNC();
    }
    MD_TR(52);
    {
        constexpr int CPL = N * N >= 64 ? N * N / 64 : 1, LANES = N * N / CPL; /* coefficients per lane; the lanes that hold some */
        const int e0 = lane * CPL;
        const bool lane_in = lane < LANES && (e0 >> LG) < area; /* (a lane's coefficients share their row: CPL <= N) */
        if (lane_in) {
            int v_[CPL];
            int16_t *qp_ = qbuf + e0;
            if constexpr (CPL == 16) {
                const uint4 a = reinterpret_cast<const uint4 *>(qp_)[0], b = reinterpret_cast<const uint4 *>(qp_)[1];
                const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
                for (int i = 0; i < 8; i++)
                    v_[2 * i] = (int16_t)(w[i] & 0xffffu), v_[2 * i + 1] = (int16_t)(w[i] >> 16);
            } else if constexpr (CPL == 4) {
                const uint2 a = *reinterpret_cast<const uint2 *>(qp_);
                v_[0] = (int16_t)(a.x & 0xffffu), v_[1] = (int16_t)(a.x >> 16), v_[2] = (int16_t)(a.y & 0xffffu), v_[3] = (int16_t)(a.y >> 16);
            } else {
                v_[0] = qp_[0];
            }
            int q_[CPL], c_[CPL];
#pragma unroll
            for (int i = 0; i < CPL; i++) {
                const bool inside = ((e0 + i) & (N - 1)) < area;
                int q, c;
                quantise(v_[i], inside, q, c);
                q_[i] = inside ? q : v_[i] /* outside the quantised area the buffer is never read */, c_[i] = c;
            }
            auto put = [&](int16_t *dst, const int (&val)[CPL]) {
                if constexpr (CPL == 16) {
                    uint32_t w[8];
#pragma unroll
                    for (int i = 0; i < 8; i++)
                        w[i] = (uint32_t)(uint16_t)val[2 * i] | ((uint32_t)(uint16_t)val[2 * i + 1] << 16);
                    reinterpret_cast<uint4 *>(dst)[0] = make_uint4(w[0], w[1], w[2], w[3]), reinterpret_cast<uint4 *>(dst)[1] = make_uint4(w[4], w[5], w[6], w[7]);
                } else if constexpr (CPL == 4) {
                    *reinterpret_cast<uint2 *>(dst) = make_uint2((uint32_t)(uint16_t)val[0] | ((uint32_t)(uint16_t)val[1] << 16), (uint32_t)(uint16_t)val[2] | ((uint32_t)(uint16_t)val[3] << 16));
                } else {
                    dst[0] = (int16_t)val[0];
                }
            };
            put(qp_, q_);
            if (recon_coeff) { /* (outside the quantised area the reconstruction buffer keeps what it held: the closed-loop decision runs without partial frequencies) */
                put(recon_coeff + e0, c_);
            }
        }
    }
    }
    MD_TR(53);
    nz = md_wave_sum(nz), d0 = md_wave_sum(d0), d1 = md_wave_sum(d1); /* the lanes beyond the unit's rows hold zeros */
    EP_WAVE_SYNC(); /* qbuf is written */
    MD_TR(54);
    const int lga = LG - pf, S4 = lga <= 2 ? 1 : 1 << (2 * (lga - 2));
    /* nz is the whole unit's count and the same in every lane: a unit without levels (most merge candidates of a B picture at these QPs) has no bits to estimate */
    const uint32_t b32 = nz ? md_coeff_bits(&cost, qbuf, N, lga, nz, type, intra_mode, component, lane, S4, &rt) : 0u;
    MdFl o;
    o.nz = nz, o.d0 = nz ? d0 : d1, o.d1 = d1, o.bits = nz ? (uint32_t)__shfl((int)b32, 0) : 0u;
    MD_TR(55);
    return o;
}

/* BOTH 8x8 chroma transform units of a 16x16 unit's survivor (FullLoop_R + CuFullDistortionFastTuMode_R, one call per plane in md_chroma_tu) as ONE 16x16 product on the
 * matrix cores: residual and transform matrix block-diagonal - diag(Cb, Cr), diag(C8, C8) - so that C X C^T = diag(C8 Cb C8^T, C8 Cr C8^T).  The register butterflies
 * keep 8 of 64 lanes busy per plane (~1.3 K issue slots each); this form transforms and quantises both planes in ~250.  The 8-point Estimate transform has no 16-bit wrap
 * level: exact for every input, no domain to check (|T1| <= 479 . 255 >> 2 < 2^15; H = T1 >> 6 within +-512, exact in f16).  src / pred: Cb's block, Cr's 1024 bytes
 * behind (the LCU's chroma source planes and the candidates' chroma predictions both lie that way); out: M.V.flc[b][0] (Cr's sums: out[4]).  Same sums, same levels in
 * qbuf (Cb's 64, then Cr's) as two md_chroma_tu calls. */
__device__ MD_LEAF_CALL void md_chroma_pair8(int lane, const uint8_t *src, const uint8_t *pred, int16_t *qbuf, int qp, int slice_type, const SvtAmdCabacCost &cost, int type,
                                             int intra_mode, int pf, const RateTables &rt, MdFl *out)
{
    constexpr int N = 8, LG = 3, fs1 = 2, fs2 = 9;
    MD_LDS(src), MD_LDS(pred), MD_LDS(qbuf), MD_LDS(&cost), MD_LDS(&rt), MD_LDS(out);
    const int pfc = pf == 2 ? 1 : pf; /* correctedPFMode (EbFullLoop.c:647-652) */
    const int qpRem = qp % 6, qpPer = qp / 6;
    const uint32_t QF = qpRem == 0 ? 26214u : qpRem == 1 ? 23302u : qpRem == 2 ? 20560u : qpRem == 3 ? 18396u : qpRem == 4 ? 16384u : 14564u;
    const int FFv = qpRem == 0 ? 40 : qpRem == 1 ? 45 : qpRem == 2 ? 51 : qpRem == 3 ? 57 : qpRem == 4 ? 64 : 72;
    const int tshift = 7 - LG, shiftedQBits = 14 + qpPer + tshift;
    const uint32_t offs = ((slice_type == 2 || slice_type == 3) ? 171u : 85u) << (shiftedQBits - 9);
    const int shiftedFFunc = qpPer > 8 ? FFv << (qpPer - 2) : FFv << qpPer;
    const int shiftNum = qpPer > 8 ? 20 - 14 - tshift - 2 : 20 - 14 - tshift, iq_offset = 1 << (shiftNum - 1);
    const int area = N >> pfc;
    const int j = lane & 15, g = lane >> 4, plane = j >> 3;
    const bool valid = (g >> 1) == plane; /* the lane's four K slots lie in its row's diagonal block */
    const uint8_t *s_ = src + plane * 1024 + (j & 7) * 32 + 4 * (g & 1), *p_ = pred + plane * 1024 + (j & 7) * N + 4 * (g & 1);
    const uint32_t a = valid ? *reinterpret_cast<const uint32_t *>(s_) : 0u, b = valid ? *reinterpret_cast<const uint32_t *>(p_) : 0u;
    const md_v4h A = md_h4((int)(a & 0xFF) - (int)(b & 0xFF), (int)((a >> 8) & 0xFF) - (int)((b >> 8) & 0xFF), (int)((a >> 16) & 0xFF) - (int)((b >> 16) & 0xFF),
                           (int)(a >> 24) - (int)(b >> 24));
    const md_v4h C = md_dct_op(10, lane);
    const md_v4f z = {0.f, 0.f, 0.f, 0.f};
    const md_v4f t1 = __builtin_amdgcn_mfma_f32_16x16x16f16(A, C, z, 0, 0, 0);
    int t[4];
#pragma unroll
    for (int i = 0; i < 4; i++)
        t[i] = (int)(int16_t)(((int)t1[i] + (1 << (fs1 - 1))) >> fs1);
    const md_v4h Hh = md_h4(t[0] >> 6, t[1] >> 6, t[2] >> 6, t[3] >> 6), Lo = md_h4(t[0] & 63, t[1] & 63, t[2] & 63, t[3] & 63);
    const md_v4f dh = __builtin_amdgcn_mfma_f32_16x16x16f16(C, Hh, z, 0, 0, 0), dl = __builtin_amdgcn_mfma_f32_16x16x16f16(C, Lo, z, 0, 0, 0);
    unsigned nz = 0, d0 = 0, d1 = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int k2 = 4 * g + i; /* coefficient (k2 & 7, j & 7) of plane j >> 3 where the lane is valid */
        const bool inside = valid && (k2 & 7) < area && (j & 7) < area;
        const int v = inside ? (int)(int16_t)((((int)dh[i] << 6) + (int)dl[i] + (1 << (fs2 - 1))) >> fs2) : 0; /* (no branch per coefficient: one outside adds zeros) */
        int tq = abs(v);
        tq = (int)__umul24((uint32_t)tq, QF);
        tq = (int)((uint32_t)tq + offs);
        tq >>= shiftedQBits;
        const int q = v < 0 ? -tq : tq; /* |q| <= 2^14 */
        const int c = clip16i((__mul24(q, shiftedFFunc) + iq_offset) >> shiftNum);
        const int df = (int16_t)(v - c);
        nz += q != 0, d0 += (uint32_t)__mul24(df, df), d1 += (uint32_t)__mul24(v, v);
        if (valid)
            qbuf[plane * 64 + (k2 & 7) * N + (j & 7)] = (int16_t)q;
    }
    /* the sums of each half of the wave (lanes 0..31: Cb's coefficients, 32..63: Cr's) */
    auto halves = [&](unsigned v, unsigned &lo, unsigned &hi) {
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false);
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false); /* row_bcast15 into rows 1 and 3 */
        lo = (uint32_t)__builtin_amdgcn_readlane((int)v, 31), hi = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
    };
    unsigned nzp[2], d0p[2], d1p[2];
    halves(nz, nzp[0], nzp[1]), halves(d0, d0p[0], d0p[1]), halves(d1, d1p[0], d1p[1]);
    EP_WAVE_SYNC(); /* qbuf is written */
    const int lga = LG - pfc, S4 = lga <= 2 ? 1 : 1 << (2 * (lga - 2));
#pragma unroll
    for (int pl = 0; pl < 2; pl++) {
        const uint32_t b32 = nzp[pl] ? md_coeff_bits(&cost, qbuf + pl * 64, N, lga, nzp[pl], type, intra_mode, 1 + pl, lane, S4, &rt) : 0u;
        const uint32_t bits = nzp[pl] ? (uint32_t)__shfl((int)b32, 0) : 0u;
        if (lane == 0) { /* md_chroma_tu's scaling of the sums: distortions >> 2 (7 - log2 N), bits << 10 >> 15 */
            constexpr int sh = 2 * (7 - LG);
            MdFl o;
            o.nz = nzp[pl];
            o.d0 = (uint32_t)(((unsigned long long)(nzp[pl] ? d0p[pl] : d1p[pl]) + (1ull << (sh - 1))) >> sh);
            o.d1 = (uint32_t)(((unsigned long long)d1p[pl] + (1ull << (sh - 1))) >> sh);
            o.bits = (uint32_t)((((unsigned long long)bits) << 10) >> 15);
            out[4 * pl] = o;
        }
    }
    EP_WAVE_SYNC();
}

/* PerformInverseTransformRecon of the winner (Codec/EbProductCodingLoop.c:1334-1414): EstimateInvTransform of the de-quantised
 * coefficients + the prediction, clipped, into the per-depth reconstruction at the unit's position (pitch 64) */
template <int N>
__device__ __forceinline__ void md_recon_unit(int lane, const int16_t *recon_coeff, const uint8_t *pred, uint8_t *dst, int16_t *tile)
{
    constexpr int P = TxRegTile<N>::PITCH;
    const int r = lane & (N - 1);
    const bool active = lane < N;
    int16_t *t = tile + (lane / N) * TxRegTile<N>::UNIT;
    int c[N];
#pragma unroll
    for (int j = 0; j < N; j++)
        c[j] = active ? (int)recon_coeff[j * N + r] : 0;
    inv_1d_regs<N>(c, 7, [&](int j, int16_t v) { t[r * P + j] = v; });
    EP_WAVE_SYNC();
#pragma unroll
    for (int k = 0; k < N; k++)
        c[k] = t[k * P + r];
    int y[N];
    inv_1d_regs<N>(c, 12, [&](int j, int16_t v) { y[j] = v; });
    if (active) {
#pragma unroll
        for (int j = 0; j < N; j++) {
            const int v = (int)pred[r * N + j] + y[j];
            dst[r * 64 + j] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
        }
    }
}

/* the luma full loop of the unit's candidate on one wave: every transform unit (four 32x32 of a 64x64 unit) -> out[tu] */
__device__ __forceinline__ void md_full_loop_cand(int lane, int N, const uint8_t *src, const uint8_t *pred, int predPitch, int16_t *recon_coeff, int16_t *tile, int16_t *qbuf,
                                                  const SvtAmdMdPicture &P, const SvtAmdCabacCost &cost, const RateTables &rt, int type, int mode, int pf, MdFl *out)
{
    if (N == 64) {
        for (int tu = 0; tu < 4; tu++) {
            const int off = ((tu & 1) << 5) + ((tu >> 1) << 5) * 64, poff = ((tu & 1) << 5) + ((tu >> 1) << 5) * predPitch;
            const MdFl o = md_full_loop_unit<32>(lane, src + off, 64, pred + poff, predPitch, nullptr, tile, qbuf, P.qp, P.slice_type, cost, type, mode, 0, pf, rt);
            if (lane == 0)
                out[tu] = o;
            EP_WAVE_SYNC();
        }
        return;
    }
    MdFl o;
    switch (N) {
    case 32: o = md_full_loop_unit<32>(lane, src, 64, pred, predPitch, recon_coeff, tile, qbuf, P.qp, P.slice_type, cost, type, mode, 0, pf, rt); break;
    case 16: o = md_full_loop_unit<16>(lane, src, 64, pred, predPitch, recon_coeff, tile, qbuf, P.qp, P.slice_type, cost, type, mode, 0, pf, rt); break;
    default: o = md_full_loop_unit<8>(lane, src, 64, pred, predPitch, recon_coeff, tile, qbuf, P.qp, P.slice_type, cost, type, mode, 0, pf, rt); break;
    }
    if (lane == 0)
        out[0] = o;
}

/* TuCalcCostLuma (Codec/EbRateDistortionCost.c:289-375) of one transform unit + the accumulation ProductFullLoop does: *ycbf, *bits, dist[2] */
__device__ __forceinline__ void md_tu_calc_cost(const SvtAmdMdPicture &P, const MdFl &o, int type, int cuSize, int T, int tuIndex, uint32_t *ycbf, unsigned long long *bits,
                                                unsigned long long dist[2])
{
    const int lgT = T == 32 ? 5 : T == 16 ? 4 : 3, dshift = cuSize == 64 ? 4 : 2 * (7 - lgT);
    const unsigned long long d0 = ((unsigned long long)o.d0 + (1ull << (dshift - 1))) >> dshift, d1 = ((unsigned long long)o.d1 + (1ull << (dshift - 1))) >> dshift;
    const unsigned long long tuBits = (((unsigned long long)o.bits) << 10) >> 15;
    const int ctx = cuSize == T;
    const unsigned long long lambda = P.full_lambda;
    const unsigned long long nzRate = (tuBits << 15) + P.rates.lumaCbfBits[5 + ctx], zRate = P.rates.lumaCbfBits[ctx];
    const unsigned long long zCost = type == MD_INTRA ? ~0ull : (d1 << 8) + ((lambda * zRate + (1u << 22)) >> 23);
    const unsigned long long nzCost = (d0 << 8) + ((lambda * nzRate + (1u << 22)) >> 23);
    const bool coded = o.nz != 0 && nzCost < zCost;
    *ycbf |= (uint32_t)coded << tuIndex;
    *bits += nzCost < zCost ? tuBits : 0;
    dist[0] += nzCost < zCost ? d0 : d1, dist[1] += d1;
}

/* one chroma transform unit of FullLoop_R + CuFullDistortionFastTuMode_R on the calling wave -> nz, the two scaled distortions, the bits */
__device__ __forceinline__ void md_chroma_tu(int lane, int T, const uint8_t *src, const uint8_t *pred, int predPitch, int16_t *tile, int16_t *qbuf, const SvtAmdMdPicture &P,
                                             const SvtAmdCabacCost &cost, const RateTables &rt, int type, int mode, int component, int pf, uint32_t *nz, unsigned long long dist[2], unsigned long long *bits)
{
    const int pfc = T == 4 ? 0 : (T == 8 && pf == 2 ? 1 : pf); /* correctedPFMode (EbFullLoop.c:647-652) */
    MdFl o;
    switch (T) {
    case 16: o = md_full_loop_unit<16>(lane, src, 32, pred, predPitch, nullptr, tile, qbuf, P.chroma_qp, P.slice_type, cost, type, mode, component, pfc, rt); break;
    case 8: o = md_full_loop_unit<8>(lane, src, 32, pred, predPitch, nullptr, tile, qbuf, P.chroma_qp, P.slice_type, cost, type, mode, component, pfc, rt); break;
    default: o = md_full_loop_unit<4>(lane, src, 32, pred, predPitch, nullptr, tile, qbuf, P.chroma_qp, P.slice_type, cost, type, mode, component, pfc, rt); break;
    }
    const int lgT = T == 16 ? 4 : T == 8 ? 3 : 2, sh = 2 * (7 - lgT);
    *nz = o.nz;
    dist[0] = ((unsigned long long)o.d0 + (1ull << (sh - 1))) >> sh, dist[1] = ((unsigned long long)o.d1 + (1ull << (sh - 1))) >> sh;
    *bits = (((unsigned long long)o.bits) << 10) >> 15;
    EP_WAVE_SYNC();
}
