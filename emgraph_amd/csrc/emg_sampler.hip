// emg_sampler.hip — the negative sampler's binding (emg_sampler_bind) and the stand-alone producer of sampled corruption codes
// (emg_corrupt_codes_sampled: emg_corrupt_codes with the positives at hand).  The draw itself: emg_sampler.hpp.
#include <stddef.h>

#include <mutex>

#include "emg_sampler.hpp"

namespace emg {

static std::mutex g_mu;
static bool g_bound = false;
static SamplerDev g_sampler;

bool sampler_current(SamplerDev* out) {
    std::lock_guard<std::mutex> g(g_mu);
    if (g_bound && out) *out = g_sampler;
    return g_bound;
}

// codes[j] as corrupt_codes_kernel's (emg_train.hip), row j corrupting positive j mod B (protocol.py:598), through the sampler
__global__ __launch_bounds__(256) void corrupt_codes_sampled_kernel(const int32_t* __restrict__ pos, int64_t B, int64_t n, int side,
                                                                    uint64_t n_choices, const int32_t* __restrict__ entities_list,
                                                                    uint64_t seed, uint64_t counter, const int32_t* __restrict__ inj_mask,
                                                                    const int32_t* __restrict__ inj_repl, int32_t* __restrict__ codes,
                                                                    const SamplerDev S) {
    __shared__ uint64_t s_coarse[kCoarseMax];
    sampler_stage_coarse(S, s_coarse);
    __syncthreads();
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    uint32_t keep, repl;
    if (inj_repl) {   // injected draws bypass the sampler, as they bypass the draw
        const uint32_t idx = (uint32_t)inj_repl[j];
        keep = inj_mask ? (uint32_t)(inj_mask[j] != 0) : 0u;
        if (side == EMG_SIDE_O) keep = 1u;
        else if (side == EMG_SIDE_S) keep = 0u;
        repl = entities_list ? (uint32_t)entities_list[idx] : idx;
    } else {
        const int64_t i = j % B;
        sampled_draw(S, s_coarse, seed, counter, (uint64_t)j, n_choices, entities_list, side, pos[3 * i + 0], pos[3 * i + 1], pos[3 * i + 2],
                     &keep, &repl);
    }
    codes[j] = (int32_t)((repl & 0x7fffffffu) | (keep << 31));
}

}  // namespace emg

using namespace emg;

extern "C" int emg_sampler_bind(const emg_sampler* s) {
    if (!s) {
        std::lock_guard<std::mutex> g(g_mu);
        g_bound = false;
        return EMG_OK;
    }
    // the structure grows at its end: a caller built against the first layout (up to `stats`) passes that size and gets that behaviour
    const int64_t size_v1 = (int64_t)offsetof(emg_sampler, pool_ptr);
    EMG_REQUIRE(s->size == size_v1 || s->size >= (int64_t)sizeof(emg_sampler), "emg_sampler_bind: size %lld is not sizeof(emg_sampler)", (long long)s->size);
    const bool has_pools = s->size >= (int64_t)sizeof(emg_sampler) && s->pool_ptr;
    EMG_REQUIRE(!has_pools || s->pool_idx, "emg_sampler_bind: pool_ptr needs pool_idx");
    EMG_REQUIRE(s->n_ent > 0 && s->n_rel > 0 && s->n_ent < ((int64_t)1 << 31) && s->n_rel < ((int64_t)1 << 31), "emg_sampler_bind: bad table sizes");
    EMG_REQUIRE(s->n_known >= 0 && (s->n_known == 0 || s->known_keys), "emg_sampler_bind: n_known keys need known_keys");
    EMG_REQUIRE(!s->stats || (reinterpret_cast<uintptr_t>(s->stats) & 7u) == 0, "emg_sampler_bind: stats must be 8-byte aligned");
    SamplerDev d{};
    d.keep_thr = s->keep_thr; d.n_ent = (uint64_t)s->n_ent; d.n_rel = (uint64_t)s->n_rel; d.stats = (unsigned long long*)s->stats;
    if (has_pools) { d.pool_ptr = s->pool_ptr; d.pool_idx = s->pool_idx; }
    if (s->n_known > 0) {
        EMG_REQUIRE(s->retries >= 1 && s->retries <= 255, "emg_sampler_bind: retries %d outside 1..255", s->retries);
        // the key (s * n_rel + p) * n_ent + o has to fit 63 bits (a signed 64-bit sort on the host side orders it the same way)
        const unsigned __int128 span = (unsigned __int128)s->n_ent * (unsigned __int128)s->n_ent * (unsigned __int128)s->n_rel;
        if (span >= ((unsigned __int128)1 << 63)) return fail(EMG_ENOSUP, "emg_sampler_bind: n_ent^2 * n_rel >= 2^63: a triple's key does not fit");
        d.known = s->known_keys; d.n_known = s->n_known; d.retries = s->retries;
        while (cdiv(s->n_known, (int64_t)1 << d.shift) > kCoarseMax) ++d.shift;
        d.n_coarse = (int32_t)cdiv(s->n_known, (int64_t)1 << d.shift);
    }
    std::lock_guard<std::mutex> g(g_mu);
    g_sampler = d;
    g_bound = true;
    return EMG_OK;
}

extern "C" int emg_sampler_bound(void) { return sampler_current(nullptr) ? 1 : 0; }

extern "C" int emg_corrupt_codes_sampled(const int32_t* pos, int64_t B, int32_t eta, int side, int64_t n_choices, const int32_t* entities_list,
                                         uint64_t seed, uint64_t draw_counter, const int32_t* inj_mask, const int32_t* inj_repl, int32_t* codes,
                                         void* stream) {
    SamplerDev S;
    if (!sampler_current(&S))   // nothing bound: the draw of emg_corrupt_codes, bit for bit
        return emg_corrupt_codes(B, eta, side, n_choices, entities_list, seed, draw_counter, inj_mask, inj_repl, codes, stream);
    EMG_REQUIRE(side >= EMG_SIDE_S && side <= EMG_SIDE_SO, "emg_corrupt_codes_sampled: bad side %d", side);
    EMG_REQUIRE(B >= 0 && eta >= 0, "emg_corrupt_codes_sampled: negative sizes");
    const int64_t n = B * eta;
    if (n == 0) return EMG_OK;
    EMG_REQUIRE(pos && codes, "emg_corrupt_codes_sampled: null pointer");
    EMG_REQUIRE(n_choices > 0 && n_choices < ((int64_t)1 << 31), "emg_corrupt_codes_sampled: n_choices=%lld out of range", (long long)n_choices);
    EMG_REQUIRE(!(side == EMG_SIDE_SO && inj_repl && !inj_mask), "emg_corrupt_codes_sampled: injected 's+o' needs inj_mask");
    hipLaunchKernelGGL(corrupt_codes_sampled_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, pos, B, n, side,
                       (uint64_t)n_choices, entities_list, seed, draw_counter, inj_mask, inj_repl, codes, S);
    EMG_LAUNCH_CHECK();
    return EMG_OK;
}
