// emg_rank_rotate.hip — RotatE 1-vs-all ranking: EXACT ranks through a half-precision prefilter.
//
// The exact RotatE kernel (emg_rank.hip::count_rotate_kernel) spends 21 VALU instructions per (query, entity, complex
// coordinate), 13 of them the correctly rounded square root.  A prefilter needs neither that root nor f32 operands, only a
// rigorous band (DESIGN.md 4.5 "Exact-fast ranking" has the proof, term by term):
//   1. the rows [re | im] of the query rows and of the entity table are multiplied by one power of two s (exact) and rounded
//      to half precision, (re_j, im_j) ADJACENT in one dword; an image value below the smallest normal half, 2^-14, is
//      written as zero (no path below depends on how an instruction treats half subnormal INPUTS).  Per row,
//      rho = sum_j |x_j s - x~_j| (moduli of the complex residuals, rounded up): the modulus is 1-Lipschitz, so rounding
//      the operands moves sum_j |q_j - e_j| by at most rho_q + rho_e;
//   2. per (row, entity, coordinate) 4.5 instructions: a packed half subtract (relative 2^-11 per component, or an absolute
//      2^-14 where a subnormal result is flushed), the 2-term dot of the difference with itself as two v_fma_mix_f32 (one
//      rounding), v_sqrt_f32 (1 ulp), an f32 add (two of them share a v_pk_add_f32);
//   3. the reference compares int(score * 1e5) with the positive's (EmbeddingModel.py:2010-2033), score = -A in the canonical
//      f32 chain (emg_chain.hpp::rotate_step): per query row two accumulator thresholds follow such that A~ < lo proves
//      "greater" (counted here) and A~ > hi proves "less" (dropped); the candidates in between are EMITTED as (row, entity)
//      pairs in the layout of emg_eval_prefilter_sad and re-scored by emg_eval_rescore_pairs(EMG_ROTATE) with the canonical chain.
// The counters, and therefore the ranks, equal the exact kernel's bit for bit; a band that is too wide costs speed only.
#include "emg_common.hpp"

#pragma clang fp contract(off)

namespace emg {

typedef _Float16 half2v __attribute__((ext_vector_type(2)));

constexpr float ROT_IMG_MAX = 32752.f;              // half of the largest half: a difference of two image values is finite
constexpr float ROT_IMG_MIN = 6.103515625e-05f;     // 2^-14, the smallest normal half
constexpr double ROT_FLUSH = 8.631674575031098e-05; // sqrt(2) 2^-14: a complex difference whose components may have been flushed
constexpr double ROT_HALF_U = 4.8828125e-04;        // 2^-11
constexpr double ROT_TINY = 8.673617379884035e-19;  // 2^-60 per coordinate: the exact chain's squares may underflow

// ONE chain step of the prefilter on complex coordinate j: acc + |q~_j - e~_j|
__device__ __forceinline__ float rotate_pre_step(uint32_t q, uint32_t e, float acc) {
    const half2v d = __builtin_bit_cast(half2v, q) - __builtin_bit_cast(half2v, e);   // v_pk_add_f16 (neg)
    // the 2-term dot as two mixed-precision FMAs (v_fma_mix_f32: half operands, f32 arithmetic, IEEE rounding): dr^2 is exact in
    // f32, so the sum carries ONE rounding.  (__builtin_amdgcn_fdot2 compiles to v_dot2c_f32_f16, whose accumulator is tied to the
    // destination: a v_mov of the zero plus hazard no-ops per step, more issue slots than these two, and no documented rounding.)
    const float m2 = __builtin_fmaf((float)d.y, (float)d.y, __builtin_fmaf((float)d.x, (float)d.x, 0.f));
    return acc + __builtin_amdgcn_sqrtf(m2);                                          // v_sqrt_f32 (1 ulp), v_add_f32
}

__device__ __forceinline__ void atomic_max_pos(double* dst, double v) {   // non-negative doubles order like their bit patterns
    atomicMax(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)__double_as_longlong(v));
}

__device__ __forceinline__ float float_up(double v) {   // smallest float >= v, v >= 0 and far below FLT_MAX
    float f = (float)v;
    if ((double)f < v) f = __uint_as_float(__float_as_uint(f) + 1u);
    return f;
}
__device__ __forceinline__ float float_down(double v) {   // largest float <= v, v > 0
    float f = (float)v;
    if ((double)f > v) f = __uint_as_float(__float_as_uint(f) - 1u);
    return f;
}

// half image value of a scaled coordinate and its residual; *bad: the value does not fit (or is not finite)
__device__ __forceinline__ uint32_t rotate_image_value(float s, double* res, bool* bad) {
    if (!(fabsf(s) <= ROT_IMG_MAX)) {   // refused (the caller takes the exact kernel); the image stays finite all the same
        *bad = true;
        s = (s != s) ? 0.f : copysignf(ROT_IMG_MAX, s);
    }
    _Float16 h = (_Float16)s;           // round to nearest even
    if (fabsf((float)h) < ROT_IMG_MIN) h = (_Float16)0.f;
    *res = (double)s - (double)(float)h;
    return (uint32_t)__builtin_bit_cast(uint16_t, h);
}

// stats[0] = max rho, stats[1] = max |x| (unscaled), stats[2] = 1 if a value was refused (device doubles, zeroed by the caller)
__global__ __launch_bounds__(256) void rotate_image_kernel(const float* __restrict__ src, int64_t n_rows, int64_t ld_src, int half,
                                                           float scale, uint32_t* __restrict__ img, int64_t ld_dw,
                                                           float* __restrict__ rho, double* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int n_dw = img ? (int)ld_dw : half;
    float amax = 0.f, rmax = 0.f;
    bool bad = false;
    for (int64_t r = wave; r < n_rows; r += n_waves) {
        const float* x = src + r * ld_src;
        double rsum = 0.0;
        for (int d = lane; d < n_dw; d += 64) {
            uint32_t w = 0u;
            if (d < half) {
                const float xr = x[d], xi = x[half + d];
                amax = fmaxf(amax, fmaxf(fabsf(xr), fabsf(xi)));
                double rr, ri;
                w = rotate_image_value(__fmul_rn(xr, scale), &rr, &bad) | (rotate_image_value(__fmul_rn(xi, scale), &ri, &bad) << 16);
                rsum += sqrt(rr * rr + ri * ri) * (1.0 + 1e-15);
            }
            if (img) img[r * ld_dw + d] = w;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) rsum += __shfl_xor(rsum, off, 64);
        const float rf = float_up(rsum * (1.0 + 1e-12));
        rmax = fmaxf(rmax, rf);
        if (lane == 0 && rho) rho[r] = rf;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off, 64));
    const bool any_bad = __any(bad);
    if (lane == 0) {
        if (rmax > 0.f) atomic_max_pos(stats, (double)rmax);
        if (amax > 0.f) atomic_max_pos(stats + 1, (double)amax);
        if (any_bad) atomic_max_pos(stats + 2, 1.0);
    }
}

// per query row: A~ < lo  =>  counted as "greater";  A~ > hi  =>  dropped;  lo <= A~ <= hi  =>  re-scored exactly.
// A~ is the prefilter's accumulator (scaled units).  With g_a = (4 + n) u 1.01 (dot 4 ulp on the square, root 1 ulp, n adds),
// h = 2^-11, F = sqrt(2) 2^-14, rho = rho_q + max rho_e the real-valued A = sum_j |q_j - e_j| satisfies
//     ((A~ / (1 + g_a) - n F) / (1 + h) - rho) / s  <=  A  <=  ((A~ / (1 - g_a) + n F) / (1 - h) + rho) / s
// and the canonical f32 chain A_c satisfies |A_c - A| <= g_s A + n 2^-60, g_s = (6 + n) u 1.01.
__global__ void rotate_thresholds_kernel(const int32_t* __restrict__ pos_int, const float* __restrict__ rho_q, int64_t n_rows, int n,
                                         float scale, const double* __restrict__ q_stats, const double* __restrict__ e_stats,
                                         float* __restrict__ lo, float* __restrict__ hi) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rows) return;
    const double p = (double)pos_int[r];
    const bool refused = q_stats[2] != 0.0 || e_stats[2] != 0.0;
    if (refused || p > 0.0 || p < -2147483000.0) {   // (a saturated comparison integer ties with every saturated candidate)
        lo[r] = 0.f;
        hi[r] = __uint_as_float(0x7f800000u);       // everything undecided: the segment overflows, the exact kernel runs
        return;
    }
    const double u = 5.9604644775390625e-08;   // 2^-24
    const double g_a = (4.0 + n) * u * 1.01, g_s = (6.0 + n) * u * 1.01, s = (double)scale;
    const double rho = (double)rho_q[r] + e_stats[0], nF = n * ROT_FLUSH, tiny = n * ROT_TINY;
    const double m = -p;   // int(-A_c 1e5) > pos  <=>  floor(fl(A_c 1e5)) < m  <=>  fl(A_c 1e5) < m
    // greater is certain when (A_upper + tiny)(1 + g_s)(1 + u) 1e5 < m
    const double X = (m * 1e-5 / ((1.0 + g_s) * (1.0 + u) * (1.0 + 1e-9)) - tiny) * s;
    const double lo_v = ((X - rho) * (1.0 - ROT_HALF_U) - nF) * (1.0 - g_a) * (1.0 - 1e-9);
    // less is certain when (A_lower - tiny)(1 - g_s)(1 - u) 1e5 >= m + 1
    const double Y = ((m + 1.0) * 1e-5 * (1.0 + 1e-9) / ((1.0 - g_s) * (1.0 - u)) + tiny) * s;
    const double hi_v = ((Y + rho) * (1.0 + ROT_HALF_U) + nF) * (1.0 + g_a) * (1.0 + 1e-9);
    lo[r] = lo_v > 1e-30 ? float_down(lo_v) : 0.f;
    hi[r] = hi_v < 1e37 ? float_up(hi_v) : __uint_as_float(0x7f800000u);
}

// ---------------------------------------------------------------------------------------------
// the count kernel, the shape of emg_rank_sad.hip::count_sad_kernel: 128 query rows x 128 entities per workgroup, 8 x 8 per
// thread, k in tiles of 8 dwords (8 complex coordinates) double-buffered in LDS (the next tile's 16-byte global loads fly
// under the arithmetic).  Per dword step a thread reads 4 x 16 bytes from LDS and issues 64 x 4 VALU instructions.
// ---------------------------------------------------------------------------------------------
struct RotPreParams {
    const uint32_t* Q; int64_t ldq;         // (re, im) half pairs, row strides in dwords
    const float* lo; const float* hi; int64_t n_rows;
    const uint32_t* ent; int64_t ld_ent; int64_t n_cand; int64_t ent_offset;
    int32_t kw;                             // dwords per row actually summed (multiple of RW)
    int32_t* cnt_gt;
    uint64_t* pairs; uint32_t* pair_count; uint32_t pair_cap; uint32_t n_segments;
    int64_t n_qb; int64_t n_cb; int64_t n_tiles; int32_t tiles_per_chunk;
    float* A; int64_t lda; float inv_scale;  // the dense form only
};

constexpr int RQ = 128, RE = 128, RW = 8, R_TILES = 32;

__global__ __launch_bounds__(256, 2) void count_rotate_pre_kernel(const RotPreParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t Qs[2][RW * RQ];
    __shared__ __attribute__((aligned(16))) uint32_t Es[2][RW * RE];
    __shared__ __attribute__((aligned(16))) float lo_s[RQ];
    __shared__ __attribute__((aligned(16))) float hi_s[RQ];
    __shared__ unsigned cnt_s[RQ];

    const int64_t id = blockIdx.x;
    const int64_t xcd = id & 7, slot = id >> 3;
    const int64_t qb = slot % P.n_qb;
    const int64_t cb = xcd + 8 * (slot / P.n_qb);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t seg = (uint32_t)blockIdx.x * 4u + (uint32_t)wave;
    if (cb >= P.n_cb) return;   // (its segments stay at count 0: the caller cleared pair_count)

    const int tq = tid & 15, te = tid >> 4;
    const int lrow = tid & 127, lh = tid >> 7;   // loader: row lrow, dwords 4 lh .. 4 lh + 3 of the k tile

    if (tid < RQ) {
        const int64_t qr = qb * RQ + tid;
        const bool ok = qr < P.n_rows;           // rows past the end are masked by row_ok below
        lo_s[tid] = ok ? P.lo[qr] : 0.f;
        hi_s[tid] = ok ? P.hi[qr] : 0.f;
        cnt_s[tid] = 0u;
    }
    const int64_t qrow_g = min(qb * RQ + lrow, P.n_rows - 1);
    const uint32_t* qptr = P.Q + qrow_g * P.ldq + 4 * lh;
    const int nkt = P.kw / RW;

    unsigned row_ok = 0u;   // bit a: this thread's a-th query row exists
#pragma unroll
    for (int a = 0; a < 8; ++a) row_ok |= (qb * RQ + (a < 4 ? 0 : 64) + 4 * tq + (a & 3) < P.n_rows) ? (1u << a) : 0u;

    unsigned cnt[8];
#pragma unroll
    for (int a = 0; a < 8; ++a) cnt[a] = 0u;
    uint64_t* const pair_base = P.pairs + (uint64_t)seg * P.pair_cap;
    unsigned pair_n = 0u, pair_over = 0u;

    const int64_t tile0 = cb * P.tiles_per_chunk;
    const int64_t tile1 = min(tile0 + (int64_t)P.tiles_per_chunk, P.n_tiles);
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        const int64_t el = min(tile * RE + lrow, P.n_cand - 1);
        const uint32_t* eptr = P.ent + el * P.ld_ent + 4 * lh;
        uint4 gq, ge;
        auto fetch = [&](int kt) {
            gq = *reinterpret_cast<const uint4*>(qptr + kt * RW);
            ge = *reinterpret_cast<const uint4*>(eptr + kt * RW);
        };
        auto stage = [&](int buf) {   // registers -> LDS, k-major
            const int kl = 4 * lh;
            Qs[buf][(kl + 0) * RQ + lrow] = gq.x; Qs[buf][(kl + 1) * RQ + lrow] = gq.y;
            Qs[buf][(kl + 2) * RQ + lrow] = gq.z; Qs[buf][(kl + 3) * RQ + lrow] = gq.w;
            Es[buf][(kl + 0) * RE + lrow] = ge.x; Es[buf][(kl + 1) * RE + lrow] = ge.y;
            Es[buf][(kl + 2) * RE + lrow] = ge.z; Es[buf][(kl + 3) * RE + lrow] = ge.w;
        };
        float acc[8][8];
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int b = 0; b < 8; ++b) acc[a][b] = 0.f;
        fetch(0);
        __syncthreads();       // (the previous tile's readers are done with buffer 0, and lo_s / hi_s are staged)
        stage(0);
        for (int kt = 0; kt < nkt; ++kt) {
            const int buf = kt & 1;
            if (kt + 1 < nkt) fetch(kt + 1);
            __syncthreads();
#pragma unroll 2
            for (int k = 0; k < RW; ++k) {
                const uint4 q0 = *reinterpret_cast<const uint4*>(&Qs[buf][k * RQ + 4 * tq]);
                const uint4 q1 = *reinterpret_cast<const uint4*>(&Qs[buf][k * RQ + 64 + 4 * tq]);
                const uint4 e0 = *reinterpret_cast<const uint4*>(&Es[buf][k * RE + 4 * te]);
                const uint4 e1 = *reinterpret_cast<const uint4*>(&Es[buf][k * RE + 64 + 4 * te]);
                const uint32_t q[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
                const uint32_t e[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
#pragma unroll
                for (int a = 0; a < 8; ++a)
#pragma unroll
                    for (int b = 0; b < 8; ++b) acc[a][b] = rotate_pre_step(q[a], e[b], acc[a][b]);
            }
            if (kt + 1 < nkt) stage(1 - buf);
        }
        // ---- epilogue: count the certain "greater", collect the undecided ------------------------------------
        const bool full = (tile + 1) * RE <= P.n_cand;   // block-uniform
        unsigned long long und = 0ull;                   // bit 8 a + b
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const int ql = (a < 4 ? 0 : 64) + 4 * tq + (a & 3);
            const float lo = lo_s[ql], hi = hi_s[ql];
            const bool rok = (row_ok >> a) & 1u;
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const bool cok = full || tile * RE + (b < 4 ? 0 : 64) + 4 * te + (b & 3) < P.n_cand;
                const float s = acc[a][b];
                cnt[a] += (unsigned)(cok && s < lo);
                und |= (cok && rok && s >= lo && s <= hi) ? (1ull << (8 * a + b)) : 0ull;
            }
        }
        if (__any(und != 0ull)) {   // wave-uniform
            const int n_l = __popcll(und);
            int incl = n_l;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int up = __shfl_up(incl, off, 64);
                if (lane >= off) incl += up;
            }
            const int total = __shfl(incl, 63, 64);
            if (pair_n + (unsigned)total > P.pair_cap) {
                pair_over = 1u;   // the caller redoes this query tile with the exact kernel
            } else {
                uint64_t* dst = pair_base + pair_n + (unsigned)(incl - n_l);
                pair_n += (unsigned)total;
                const uint64_t row0 = (uint64_t)(qb * RQ + 4 * tq);
                const uint64_t col0 = (uint64_t)(P.ent_offset + tile * RE + 4 * te);
                while (und) {
                    const int bit = __ffsll((long long)und) - 1;
                    und &= und - 1ull;
                    const int a = bit >> 3, b = bit & 7;
                    *dst++ = ((row0 + (uint64_t)((a < 4 ? 0 : 64) + (a & 3))) << 32) |
                             (uint32_t)(col0 + (uint64_t)((b < 4 ? 0 : 64) + (b & 3)));
                }
            }
        }
    }
    if (lane == 0) {
        P.pair_count[seg] = pair_n;
        if (pair_over) atomicOr(P.pair_count + P.n_segments, 1u);
    }
    // 16 threads share a query row
#pragma unroll
    for (int a = 0; a < 8; ++a)
        if (cnt[a]) atomicAdd(&cnt_s[(a < 4 ? 0 : 64) + 4 * tq + (a & 3)], cnt[a]);
    __syncthreads();
    if (tid < RQ) {
        const int64_t qr = qb * RQ + tid;
        const unsigned c = cnt_s[tid];
        if (qr < P.n_rows && c) atomicAdd(&P.cnt_gt[qr], (int)c);
    }
}

// the dense debug form: one thread per (row, candidate), the same chain through the same device function, j ascending
__global__ __launch_bounds__(256) void rotate_pre_dense_kernel(const RotPreParams P) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n_rows * P.n_cand) return;
    const int64_t r = i / P.n_cand, c = i % P.n_cand;
    const uint32_t* q = P.Q + r * P.ldq;
    const uint32_t* e = P.ent + c * P.ld_ent;
    float acc = 0.f;
    for (int k = 0; k < P.kw; ++k) acc = rotate_pre_step(q[k], e[k], acc);
    P.A[r * P.lda + c] = __fmul_rn(acc, P.inv_scale);
}

static int64_t rot_pre_blocks(int64_t n_rows, int64_t n_cand) {
    const int64_t n_qb = cdiv(n_rows, RQ), n_cb = cdiv(cdiv(n_cand, RE), R_TILES);
    return 8 * n_qb * cdiv(n_cb, 8);
}

static bool pow2_scale(float s) {
    int e = 0;
    return s > 0.f && s <= 16777216.f && s >= 1.f && frexpf(s, &e) == 0.5f;
}

}  // namespace emg

using namespace emg;

extern "C" int64_t emg_eval_rotate_ld(int32_t k_int) { return k_int <= 0 ? 0 : (int64_t)(k_int + 2 * RW - 1) / (2 * RW) * (2 * RW); }

extern "C" int emg_eval_rotate_image(const float* src, int64_t n_rows, int64_t ld_src, int32_t k_int, float scale, void* img_f16,
                                     int64_t ld_img, float* rho, double* stats, int32_t check, void* stream) {
    EMG_REQUIRE(n_rows >= 0 && k_int > 0 && k_int % 2 == 0 && ld_src >= k_int, "emg_eval_rotate_image: bad sizes (k_int even, ld_src >= k_int)");
    EMG_REQUIRE(pow2_scale(scale), "emg_eval_rotate_image: scale must be a power of two in [1, 2^24]");
    EMG_REQUIRE(stats, "emg_eval_rotate_image: null stats");
    EMG_REQUIRE(!img_f16 || (ld_img >= emg_eval_rotate_ld(k_int) && ld_img % 8 == 0 && aligned16(img_f16) && rho),
                "emg_eval_rotate_image: the image needs 16-byte aligned rows of ld_img %% 8 == 0, at least emg_eval_rotate_ld(k_int) = %lld, columns and rho",
                (long long)emg_eval_rotate_ld(k_int));
    hipStream_t st = (hipStream_t)stream;
    EMG_HIP(hipMemsetAsync(stats, 0, 3 * sizeof(double), st));
    if (n_rows > 0) {
        EMG_REQUIRE(src, "emg_eval_rotate_image: null pointer");
        const int64_t b = cdiv(n_rows, 4 * 4);   // 4 rows per wave and trip
        hipLaunchKernelGGL(rotate_image_kernel, dim3((unsigned)(b > 16384 ? 16384 : b)), dim3(256), 0, st, src, n_rows, ld_src, (int)(k_int / 2),
                           scale, (uint32_t*)img_f16, ld_img / 2, rho, stats);
        EMG_LAUNCH_CHECK();
    }
    if (check) {   // the verdict of the device-side range reduction
        double h[3] = {0.0, 0.0, 0.0};
        EMG_HIP(hipMemcpyAsync(h, stats, sizeof(h), hipMemcpyDeviceToHost, st));
        EMG_HIP(hipStreamSynchronize(st));
        if (h[2] != 0.0)
            return fail(EMG_ENOSUP, "emg_eval_rotate_image: an entry is not finite or, scaled, exceeds %g (largest finite magnitude %g): the exact kernel ranks this table",
                        (double)ROT_IMG_MAX, h[1]);
    }
    return EMG_OK;
}

extern "C" int emg_eval_rotate_thresholds(const int32_t* pos_int, const float* rho_q, int64_t n_rows, int32_t k_int, float scale,
                                          const double* q_stats, const double* ent_stats, float* lo, float* hi, void* stream) {
    EMG_REQUIRE(n_rows >= 0 && k_int > 0 && k_int % 2 == 0, "emg_eval_rotate_thresholds: bad sizes");
    EMG_REQUIRE(pow2_scale(scale), "emg_eval_rotate_thresholds: scale must be a power of two in [1, 2^24]");
    if (n_rows == 0) return EMG_OK;
    EMG_REQUIRE(pos_int && rho_q && q_stats && ent_stats && lo && hi, "emg_eval_rotate_thresholds: null pointer");
    hipLaunchKernelGGL(rotate_thresholds_kernel, dim3((unsigned)cdiv(n_rows, 256)), dim3(256), 0, (hipStream_t)stream, pos_int, rho_q,
                       n_rows, (int)(k_int / 2), scale, q_stats, ent_stats, lo, hi);
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}

extern "C" int64_t emg_eval_prefilter_rotate_segments(int64_t n_rows, int64_t n_cand) {
    return (n_rows <= 0 || n_cand <= 0) ? 0 : 4 * rot_pre_blocks(n_rows, n_cand);
}

static int rot_pre_images(const char* what, const void* q_f16, int64_t ldq, const void* ent_f16, int64_t ld_ent, int32_t k_int, RotPreParams& P) {
    EMG_REQUIRE(k_int > 0 && k_int % 2 == 0, "%s: k_int must be even", what);
    const int64_t kp = emg_eval_rotate_ld(k_int);
    EMG_REQUIRE(q_f16 && ent_f16 && ldq >= kp && ld_ent >= kp && ldq % 8 == 0 && ld_ent % 8 == 0 && aligned16(q_f16) && aligned16(ent_f16),
                "%s: rows must be 16-byte aligned half images (emg_eval_rotate_image) of at least emg_eval_rotate_ld(k_int) = %lld columns", what,
                (long long)kp);
    P.Q = (const uint32_t*)q_f16; P.ldq = ldq / 2; P.ent = (const uint32_t*)ent_f16; P.ld_ent = ld_ent / 2; P.kw = (int32_t)(kp / 2);
    return EMG_OK;
}

extern "C" int emg_eval_prefilter_rotate(const void* q_f16, int64_t ldq, const float* lo, const float* hi, int64_t n_rows,
                                         const void* ent_f16, int64_t n_cand, int64_t ld_ent, int64_t ent_offset, int32_t k_int,
                                         int32_t* cnt_gt, uint64_t* pairs, uint32_t* pair_count, int64_t pairs_capacity, void* stream) {
    EMG_REQUIRE(n_rows >= 0 && n_cand >= 0 && k_int > 0 && ent_offset >= 0, "emg_eval_prefilter_rotate: bad sizes");
    if (n_rows == 0 || n_cand == 0) return EMG_OK;
    EMG_REQUIRE(lo && hi && cnt_gt && pairs && pair_count, "emg_eval_prefilter_rotate: null pointer");
    RotPreParams P{};
    int rc = rot_pre_images("emg_eval_prefilter_rotate", q_f16, ldq, ent_f16, ld_ent, k_int, P);
    if (rc != EMG_OK) return rc;
    EMG_REQUIRE(n_rows < ((int64_t)1 << 31) && ent_offset + n_cand < ((int64_t)1 << 31), "emg_eval_prefilter_rotate: ids must fit 31 bits");
    const int64_t n_seg = emg_eval_prefilter_rotate_segments(n_rows, n_cand);
    EMG_REQUIRE(pairs_capacity >= n_seg && pairs_capacity / n_seg < ((int64_t)1 << 31),
                "emg_eval_prefilter_rotate: pair buffer smaller than one entry per wave (%lld)", (long long)n_seg);
    P.lo = lo; P.hi = hi; P.n_rows = n_rows; P.n_cand = n_cand; P.ent_offset = ent_offset; P.cnt_gt = cnt_gt;
    P.pairs = pairs; P.pair_count = pair_count; P.pair_cap = (uint32_t)(pairs_capacity / n_seg); P.n_segments = (uint32_t)n_seg;
    P.n_qb = cdiv(n_rows, RQ); P.n_tiles = cdiv(n_cand, RE); P.tiles_per_chunk = R_TILES; P.n_cb = cdiv(P.n_tiles, R_TILES);
    const int64_t blocks = rot_pre_blocks(n_rows, n_cand);
    EMG_REQUIRE(blocks < ((int64_t)1 << 29), "emg_eval_prefilter_rotate: grid too large");
    hipStream_t st = (hipStream_t)stream;
    EMG_HIP(hipMemsetAsync(pair_count, 0, (size_t)(n_seg + 1) * sizeof(uint32_t), st));
    hipLaunchKernelGGL(count_rotate_pre_kernel, dim3((unsigned)blocks), dim3(256), 0, st, P);
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}

extern "C" int emg_eval_prefilter_rotate_dense(const void* q_f16, int64_t ldq, int64_t n_rows, const void* ent_f16, int64_t n_cand,
                                               int64_t ld_ent, int32_t k_int, float scale, float* A, int64_t lda, void* stream) {
    EMG_REQUIRE(n_rows >= 0 && n_cand >= 0 && k_int > 0 && lda >= n_cand, "emg_eval_prefilter_rotate_dense: bad sizes");
    EMG_REQUIRE(pow2_scale(scale), "emg_eval_prefilter_rotate_dense: scale must be a power of two in [1, 2^24]");
    if (n_rows == 0 || n_cand == 0) return EMG_OK;
    EMG_REQUIRE(A, "emg_eval_prefilter_rotate_dense: null pointer");
    RotPreParams P{};
    int rc = rot_pre_images("emg_eval_prefilter_rotate_dense", q_f16, ldq, ent_f16, ld_ent, k_int, P);
    if (rc != EMG_OK) return rc;
    P.n_rows = n_rows; P.n_cand = n_cand; P.A = A; P.lda = lda; P.inv_scale = 1.0f / scale;
    const int64_t blocks = cdiv(n_rows * n_cand, 256);
    EMG_REQUIRE(blocks < ((int64_t)1 << 31), "emg_eval_prefilter_rotate_dense: a debug form for small sizes");
    hipLaunchKernelGGL(rotate_pre_dense_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, P);
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}
