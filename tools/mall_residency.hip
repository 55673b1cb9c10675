// Infinity Cache (MALL) residency under per-instruction cache policy (tools/mall_residency, standalone):
//   residency  write a set R (80..240 MB) with plain stores, stream ~0.88 GB of random 1600-byte rows past it with
//              ONE policy (loads, or stores), then time a random re-gather of R against R just written (hot) and R
//              after a 2 GiB plain sweep (cold)
//   stepmix    mix23 with a resident subset: per group of 23 rows, 16 singleton rows read and written back in place
//              with policy P, 7 rows read from a 66 MB multi-hit subset (plain), 5 contribution rows written to a
//              131 MB buffer (policy C); then an apply-like consumer gathers the contribution rows and the multi-hit
//              rows and writes the multi-hit rows back. Timed: the mix and the consumer, per policy set
// policies: plain, nt, sc1, sc0 sc1, sc0 sc1 nt (vector-memory bits of global_load/store_dwordx4)
// build: hipcc --offload-arch=gfx950 -O3 -o tools/mall_residency tools/mall_residency.hip
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

typedef float vf4 __attribute__((ext_vector_type(4)));

enum { P_PLAIN = 0, P_NT = 1, P_SC1 = 2, P_SC01 = 3, P_SC01NT = 4, NPOL = 5 };
static const char* kPolName[NPOL] = {"plain", "nt", "sc1", "sc0_sc1", "sc0_sc1_nt"};

// issue only: wait() before the value is used
template <int P>
__device__ __forceinline__ vf4 gld(const float* p) {
    vf4 v;
    if constexpr (P == P_PLAIN) asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v) : "v"(p) : "memory");
    else if constexpr (P == P_NT) asm volatile("global_load_dwordx4 %0, %1, off nt" : "=v"(v) : "v"(p) : "memory");
    else if constexpr (P == P_SC1) asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(v) : "v"(p) : "memory");
    else if constexpr (P == P_SC01) asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1" : "=v"(v) : "v"(p) : "memory");
    else asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1 nt" : "=v"(v) : "v"(p) : "memory");
    return v;
}
template <int P>
__device__ __forceinline__ void gst(float* p, vf4 v) {
    if constexpr (P == P_PLAIN) asm volatile("global_store_dwordx4 %0, %1, off" ::"v"(p), "v"(v) : "memory");
    else if constexpr (P == P_NT) asm volatile("global_store_dwordx4 %0, %1, off nt" ::"v"(p), "v"(v) : "memory");
    else if constexpr (P == P_SC1) asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
    else if constexpr (P == P_SC01) asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" ::"v"(p), "v"(v) : "memory");
    else asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1 nt" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void landed(vf4& v) { asm volatile("" : "+v"(v)); }

__global__ __launch_bounds__(256) void sweep(vf4* __restrict__ dst, size_t n) {   // plain write
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * 256;
    const vf4 v = {1.f, 2.f, 3.f, 4.f};
    for (; i < n; i += stride) dst[i] = v;
}

// one wave per row (100 float4 chunks: lanes 0..63 chunk lane, lanes 0..35 chunk 64 + lane), 4 rows in flight per wave.
// MODE 0: read rows with policy P; MODE 1: write rows with policy P
template <int MODE, int P>
__global__ __launch_bounds__(256) void rows(float* __restrict__ table, const int32_t* __restrict__ ids, int64_t n, int64_t ld,
                                            float* out) {
    const int lane = threadIdx.x & 63;
    const bool second = lane < 36;
    const int64_t wave = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int64_t nw = (int64_t)gridDim.x * 4;
    vf4 acc = {0, 0, 0, 0};
    for (int64_t r0 = wave * 4; r0 < n; r0 += nw * 4) {
        float* p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] = table + (int64_t)ids[r0 + u < n ? r0 + u : n - 1] * ld;
        if (MODE == 0) {
            vf4 a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = gld<P>(p[u] + 4 * lane);
                b[u] = second ? gld<P>(p[u] + 4 * (64 + lane)) : vf4{0, 0, 0, 0};
            }
            wait();
#pragma unroll
            for (int u = 0; u < 4; ++u) { landed(a[u]); landed(b[u]); acc += a[u] + b[u]; }
        } else {
            const vf4 v = {1.f, 2.f, 3.f, (float)r0};
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (r0 + u < n) {
                    gst<P>(p[u] + 4 * lane, v);
                    if (second) gst<P>(p[u] + 4 * (64 + lane), v);
                }
        }
    }
    if (acc.x + acc.y + acc.z + acc.w == 1.2345f) out[0] = 1.f;
}

// per group g (one wave): rows 0..15 singletons (ids), read and written back in place with policy IP; rows 16..22 from
// the multi-hit subset (hot ids), read plain; rows 16..20 emit a contribution row to cbuf[5 g + j - 16] with policy CP
template <int IP, int CP>
__global__ __launch_bounds__(256) void mix23(float* __restrict__ table, const int32_t* __restrict__ ids, int64_t groups, int64_t ld,
                                             float* __restrict__ cbuf) {
    const int lane = threadIdx.x & 63;
    const int64_t g = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (g >= groups) return;
    const bool second = lane < 36;
    vf4 qa = {0, 0, 0, 0}, qb = qa;
    for (int j0 = 0; j0 < 23; j0 += 4) {
        vf4 a[4], b[4];
        float* p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] = table + (int64_t)ids[g * 23 + (j0 + u < 23 ? j0 + u : 22)] * ld;
        if (j0 < 16) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = gld<IP>(p[u] + 4 * lane);
                b[u] = second ? gld<IP>(p[u] + 4 * (64 + lane)) : vf4{0, 0, 0, 0};
            }
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = gld<P_PLAIN>(p[u] + 4 * lane);
                b[u] = second ? gld<P_PLAIN>(p[u] + 4 * (64 + lane)) : vf4{0, 0, 0, 0};
            }
        }
        wait();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            landed(a[u]); landed(b[u]);
            const int j = j0 + u;
            if (j >= 23) break;
            qa += a[u]; qb += b[u];
            if (j < 16) {
                gst<IP>(p[u] + 4 * lane, a[u] * 1.0001f);
                if (second) gst<IP>(p[u] + 4 * (64 + lane), b[u] * 1.0001f);
            } else if (j < 21) {
                float* s = cbuf + (g * 5 + (j - 16)) * ld;
                gst<CP>(s + 4 * lane, qa);
                if (second) gst<CP>(s + 4 * (64 + lane), qb);
            }
        }
    }
}

// apply-like consumer: wave w gathers contribution rows cperm[w * PER .. w * PER + PER - 1] and adds them into the
// multi-hit row hot[w], written back plain (PER = contribution rows / multi-hit rows, rounded down)
__global__ __launch_bounds__(256) void consume(float* __restrict__ table, const int32_t* __restrict__ hot, int64_t nhot,
                                               const float* __restrict__ cbuf, const int32_t* __restrict__ cperm, int per, int64_t ld) {
    const int lane = threadIdx.x & 63;
    const int64_t w = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (w >= nhot) return;
    const bool second = lane < 36;
    float* row = table + (int64_t)hot[w] * ld;
    vf4 a = gld<P_PLAIN>(row + 4 * lane);
    vf4 b = second ? gld<P_PLAIN>(row + 4 * (64 + lane)) : vf4{0, 0, 0, 0};
    for (int j0 = 0; j0 < per; j0 += 4) {
        vf4 x[4], y[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            x[u] = y[u] = vf4{0, 0, 0, 0};
            if (j0 + u < per) {
                const float* c = cbuf + (int64_t)cperm[w * per + j0 + u] * ld;
                x[u] = gld<P_PLAIN>(c + 4 * lane);
                if (second) y[u] = gld<P_PLAIN>(c + 4 * (64 + lane));
            }
        }
        wait();
        landed(a); landed(b);
#pragma unroll
        for (int u = 0; u < 4; ++u) { landed(x[u]); landed(y[u]); if (j0 + u < per) { a += x[u]; b += y[u]; } }
    }
    wait();
    landed(a); landed(b);
    gst<P_PLAIN>(row + 4 * lane, a);
    if (second) gst<P_PLAIN>(row + 4 * (64 + lane), b);
}

static hipEvent_t E0, E1;
template <typename F>
static double once_ms(F f) {
    CK(hipEventRecord(E0));
    f();
    CK(hipEventRecord(E1));
    CK(hipEventSynchronize(E1));
    float ms;
    CK(hipEventElapsedTime(&ms, E0, E1));
    return ms;
}
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

static uint64_t rs = 88172645463325252ull;
static uint64_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs; }

template <int MODE, int P>
static void launch_rows(float* t, const int32_t* ids, int64_t n, int64_t ld, float* out) {
    hipLaunchKernelGGL((rows<MODE, P>), dim3((unsigned)((n + 15) / 16)), dim3(256), 0, 0, t, ids, n, ld, out);
}
typedef void (*RowsFn)(float*, const int32_t*, int64_t, int64_t, float*);
template <int IP, int CP>
static void launch_mix(float* t, const int32_t* ids, int64_t groups, int64_t ld, float* cbuf) {
    hipLaunchKernelGGL((mix23<IP, CP>), dim3((unsigned)((groups + 3) / 4)), dim3(256), 0, 0, t, ids, groups, ld, cbuf);
}
typedef void (*MixFn)(float*, const int32_t*, int64_t, int64_t, float*);

int main(int argc, char** argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 5;
    const int64_t n_ent = 1000000, ld = 400, rowb = 1600;
    const size_t nflush = (size_t)1 << 27;   // float4: 2 GiB
    float *table, *rset, *out;
    vf4* flush;
    CK(hipMalloc(&table, n_ent * rowb));
    CK(hipMalloc(&flush, nflush * 16));
    const int64_t rmax = 240000000 / rowb;
    CK(hipMalloc(&rset, rmax * rowb));
    CK(hipMalloc(&out, 64));
    CK(hipMemset(table, 0, n_ent * rowb));
    CK(hipMemset(rset, 0, rmax * rowb));
    CK(hipEventCreate(&E0)); CK(hipEventCreate(&E1));
    auto do_flush = [&] { hipLaunchKernelGGL(sweep, dim3(8192), dim3(256), 0, 0, flush, nflush); };

    // stream: 550 000 random rows of the 1.6 GB table (0.88 GB)
    const int64_t nstream = 550000;
    std::vector<int32_t> h(nstream);
    for (auto& v : h) v = (int32_t)(rnd() % n_ent);
    int32_t *sids, *rids;
    CK(hipMalloc(&sids, nstream * 4));
    CK(hipMemcpy(sids, h.data(), nstream * 4, hipMemcpyHostToDevice));
    std::vector<int32_t> rp(rmax);
    for (int64_t i = 0; i < rmax; ++i) rp[i] = (int32_t)i;
    CK(hipMalloc(&rids, rmax * 4));

    RowsFn sload[NPOL] = {launch_rows<0, 0>, launch_rows<0, 1>, launch_rows<0, 2>, launch_rows<0, 3>, launch_rows<0, 4>};
    RowsFn sstore[NPOL] = {launch_rows<1, 0>, launch_rows<1, 1>, launch_rows<1, 2>, launch_rows<1, 3>, launch_rows<1, 4>};

    printf("{\n \"residency\": [\n");
    bool first = true;
    for (int rmb : {80, 150, 200, 240}) {
        const int64_t nr = (int64_t)rmb * 1000000 / rowb;
        std::vector<int32_t> perm(rp.begin(), rp.begin() + nr);
        for (int64_t i = nr - 1; i > 0; --i) std::swap(perm[i], perm[rnd() % (i + 1)]);
        CK(hipMemcpy(rids, perm.data(), nr * 4, hipMemcpyHostToDevice));
        auto write_r = [&] { hipLaunchKernelGGL(sweep, dim3(4096), dim3(256), 0, 0, (vf4*)rset, (size_t)nr * rowb / 16); };
        auto gather_r = [&] { launch_rows<0, P_PLAIN>(rset, rids, nr, ld, out); };
        std::vector<double> hot, cold;
        for (int r = 0; r < reps; ++r) {
            do_flush(); write_r();
            hot.push_back(once_ms(gather_r));
            write_r(); do_flush();
            cold.push_back(once_ms(gather_r));
        }
        const double th = median(hot), tc = median(cold);
        printf("%s  {\"R_MB\": %d, \"hot_ms\": %.4f, \"cold_ms\": %.4f, \"hot_TBps\": %.2f, \"cold_TBps\": %.2f",
               first ? "" : ",\n", rmb, th, tc, nr * rowb / th / 1e9, nr * rowb / tc / 1e9);
        first = false;
        for (int op = 0; op < 2; ++op)
            for (int p = 0; p < NPOL; ++p) {
                std::vector<double> g, s;
                for (int r = 0; r < reps; ++r) {
                    do_flush(); write_r();
                    s.push_back(once_ms([&] { (op ? sstore : sload)[p](table, sids, nstream, ld, out); }));
                    g.push_back(once_ms(gather_r));
                }
                const double tg = median(g);
                // resident share: 1 at the hot time, 0 at the cold time
                printf(", \"%s_%s_stream_ms\": %.4f, \"%s_%s_regather_ms\": %.4f, \"%s_%s_resident\": %.2f", op ? "store" : "load",
                       kPolName[p], median(s), op ? "store" : "load", kPolName[p], tg, op ? "store" : "load", kPolName[p],
                       (tc - tg) / (tc - th));
            }
        printf("}");
        fflush(stdout);
    }
    printf("\n ],\n");

    // step mix: 16384 groups; singleton rows 0..15 unique rows outside the multi-hit subset; rows 16..22 drawn from a
    // subset of 40 960 rows (66 MB); 81 920 contribution rows (131 MB), two per multi-hit row in the consumer
    const int64_t groups = 16384, nhot = 40960, ncon = groups * 5;
    std::vector<int32_t> all(n_ent);
    for (int64_t i = 0; i < n_ent; ++i) all[i] = (int32_t)i;
    for (int64_t i = n_ent - 1; i > 0; --i) std::swap(all[i], all[rnd() % (i + 1)]);
    std::vector<int32_t> mids(groups * 23);
    int64_t next = nhot;
    for (int64_t g = 0; g < groups; ++g)
        for (int j = 0; j < 23; ++j) mids[g * 23 + j] = j < 16 ? all[next++] : all[rnd() % nhot];
    int32_t *dmids, *dhot, *dcperm;
    float* cbuf;
    const int per = (int)(ncon / nhot);
    std::vector<int32_t> cperm(ncon);
    for (int64_t i = 0; i < ncon; ++i) cperm[i] = (int32_t)i;
    for (int64_t i = ncon - 1; i > 0; --i) std::swap(cperm[i], cperm[rnd() % (i + 1)]);
    CK(hipMalloc(&dmids, mids.size() * 4));
    CK(hipMalloc(&dhot, nhot * 4));
    CK(hipMalloc(&dcperm, ncon * 4));
    CK(hipMalloc(&cbuf, ncon * rowb));
    CK(hipMemcpy(dmids, mids.data(), mids.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dhot, all.data(), nhot * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dcperm, cperm.data(), ncon * 4, hipMemcpyHostToDevice));
    CK(hipMemset(cbuf, 0, ncon * rowb));
    auto consumer = [&] { hipLaunchKernelGGL(consume, dim3((unsigned)((nhot + 3) / 4)), dim3(256), 0, 0, table, dhot, nhot, cbuf, dcperm, per, ld); };
    struct Set { const char* name; MixFn f; };
    const Set sets[] = {
        {"today_inplace_plain_contrib_nt", launch_mix<P_PLAIN, P_NT>},
        {"inplace_plain_contrib_plain", launch_mix<P_PLAIN, P_PLAIN>},
        {"inplace_nt_contrib_plain", launch_mix<P_NT, P_PLAIN>},
        {"inplace_sc1_contrib_plain", launch_mix<P_SC1, P_PLAIN>},
        {"inplace_sc0sc1_contrib_plain", launch_mix<P_SC01, P_PLAIN>},
        {"inplace_sc0sc1nt_contrib_plain", launch_mix<P_SC01NT, P_PLAIN>},
        {"inplace_nt_contrib_nt", launch_mix<P_NT, P_NT>},
    };
    const double mixb = (double)groups * (23 + 16 + 5) * rowb, conb = (double)(nhot * 2 + (int64_t)per * nhot) * rowb;
    printf(" \"stepmix\": {\"groups\": %lld, \"multi_hit_rows\": %lld, \"contribution_rows\": %lld, \"mix_bytes\": %.0f, \"consumer_bytes\": %.0f",
           (long long)groups, (long long)nhot, (long long)ncon, mixb, conb);
    {
        std::vector<double> cold, hot;
        for (int r = 0; r < reps; ++r) {
            do_flush();
            cold.push_back(once_ms(consumer));
            hot.push_back(once_ms(consumer));
        }
        printf(",\n  \"consumer_cold_ms\": %.4f, \"consumer_hot_ms\": %.4f", median(cold), median(hot));
    }
    for (const Set& s : sets) {
        std::vector<double> m, c;
        for (int r = 0; r < reps; ++r) {
            do_flush();
            m.push_back(once_ms([&] { s.f(table, dmids, groups, ld, cbuf); }));
            c.push_back(once_ms(consumer));
        }
        printf(",\n  \"%s_mix_ms\": %.4f, \"%s_consumer_ms\": %.4f", s.name, median(m), s.name, median(c));
        fflush(stdout);
    }
    printf("\n },\n \"note\": \"median of %d; rows are 1600 B; resident = (cold - t) / (cold - hot) of the re-gather\"\n}\n", reps);
    CK(hipDeviceSynchronize());
    return 0;
}
