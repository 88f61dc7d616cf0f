// Exact order statistics of z-ranges of one image channel: most-significant-byte-first radix select.
// replaces: the sort behind `np.percentile(plane, (lower, upper))` of the reference's import loop and of
// importer.calc_intensity_bounds (magmap/io/importer.py:1367-1377, 1415-1444) -- the host assembles the percentile
// from the two order statistics either side of its virtual index, exactly as NumPy does.
//
// One level = one streaming pass (os_count_kernel) + one small kernel (os_select_kernel):
//   count : every workgroup walks one chunk of ONE group with 16-byte loads and counts byte `level` of the keys whose
//           higher bytes equal the current prefix of one of the group's (up to four distinct) ranks: a private
//           histogram per wave in LDS; a lane first gathers the elements of its own load and the wave folds equal
//           entries into one add (microscope images have narrow histograms: at level 0 nearly every lane hits the
//           same one or two bins), a wide histogram goes straight to LDS atomics; then the workgroup's non-zero
//           bins go to the group's 64-bit histogram in global memory;
//   select: one workgroup per group, one wave per rank: scan the 256 bins, pick the bin, update prefix and remaining
//           rank, clear the histograms, work out which ranks still share a prefix (they share a histogram).
// Traffic: levels x bytes of the channel (1 level for uint8, 2 for uint16 / int16, 4 for float32, 8 for float64).
// Everything is queued on the caller's stream; nothing waits for the device.
#include <algorithm>

#include "mmx_common.h"

namespace {

constexpr int kRanks = 4;
constexpr int kBins = 256;
constexpr int kWaves = MMX_WG / 64;
constexpr int64_t kChunkBytes = 256 << 10;     // contiguous voxels one workgroup walks
constexpr int64_t kChunkStrided = 64 << 10;    // voxels one workgroup walks through a strided channel
constexpr int kFoldMin = 16;                   // lanes the first fold of a load must take for the rest of it to fold too

// per-group state between the levels (device workspace, behind the histograms)
struct os_state {
    unsigned long long prefix[kRanks];   // the key's bytes chosen so far (as the key's top `level` bytes, right-aligned)
    unsigned long long rem[kRanks];      // rank among the keys that share the prefix
    unsigned long long uprefix[kRanks];  // distinct prefixes = histograms in flight (unused: ~0, matches no key)
    int32_t slot[kRanks];                // histogram of rank r
    int32_t n_uniq;
    int32_t _pad[3];
};
static_assert(sizeof(os_state) == 128, "os_state layout");

// the elements of one 16-byte load
template <typename T> struct os_vec { static constexpr int n = 16 / (int)sizeof(T); };
template <typename T> __device__ __forceinline__ T os_elem(const uint4& q, int j);
template <> __device__ __forceinline__ uint8_t os_elem<uint8_t>(const uint4& q, int j)
{
    const uint32_t w = j < 4 ? q.x : j < 8 ? q.y : j < 12 ? q.z : q.w;
    return (uint8_t)(w >> (8 * (j & 3)));
}
template <> __device__ __forceinline__ uint16_t os_elem<uint16_t>(const uint4& q, int j)
{
    const uint32_t w = j < 2 ? q.x : j < 4 ? q.y : j < 6 ? q.z : q.w;
    return (uint16_t)(w >> (16 * (j & 1)));
}
template <> __device__ __forceinline__ int16_t os_elem<int16_t>(const uint4& q, int j)
{
    return (int16_t)os_elem<uint16_t>(q, j);
}
template <> __device__ __forceinline__ float os_elem<float>(const uint4& q, int j)
{
    return __uint_as_float(j == 0 ? q.x : j == 1 ? q.y : j == 2 ? q.z : q.w);
}
template <> __device__ __forceinline__ double os_elem<double>(const uint4& q, int j)
{
    const unsigned long long b = j == 0 ? ((unsigned long long)q.y << 32) | q.x : ((unsigned long long)q.w << 32) | q.z;
    return __longlong_as_double((long long)b);
}

// `w` equal entries (histogram slot * 256 + bin; < 0: the key shares no prefix in flight) per lane into the wave's
// private histogram.  Lanes with the entry of the first active lane are folded into one add of their summed weights
// (one ballot per bit of the weight), ROUNDS times; what is left takes LDS atomics.  Returns how many lanes the first
// round took (64 when no lane had an entry; uniform).
template <int WBITS, int ROUNDS>
__device__ __forceinline__ int os_fold(uint32_t* wh, int idx, int w, int lane)
{
    bool active = idx >= 0;
    int took = 64;
#pragma unroll
    for (int round = 0; round < ROUNDS; ++round) {
        const unsigned long long act = __ballot(active);
        if (act == 0) break;                                               // (uniform)
        const int lead = (int)__ffsll((long long)act) - 1;
        const int first = __builtin_amdgcn_readlane(idx, lead);
        const bool same = active && idx == first;
        int c = 0;
#pragma unroll
        for (int k = 0; k < WBITS; ++k) c += (int)__popcll(__ballot(same && ((w >> k) & 1))) << k;
        if (lane == lead) wh[first] += (uint32_t)c;
        if (round == 0) took = (int)__popcll(__ballot(same));
        active = active && !same;
    }
    if (active) atomicAdd(&wh[idx], (uint32_t)w);
    return took;
}

__device__ __forceinline__ void os_add(uint32_t* wh, int idx)
{
    if (idx >= 0) atomicAdd(&wh[idx], 1u);
}

// bits of the largest weight a lane can bring (the elements of one 16-byte load)
template <int VE> struct os_wbits { static constexpr int n = VE >= 16 ? 5 : VE >= 8 ? 4 : VE >= 4 ? 3 : 2; };

// L0: the first level -- no byte chosen yet, every key counts, into histogram 0
template <typename T, bool L0>
__global__ void __launch_bounds__(MMX_WG)
os_count_kernel(const T* __restrict__ vol, int64_t sz, int64_t sy, int64_t sx, int64_t ny, int64_t nx, int contiguous,
                const mmx_rank_group* __restrict__ groups, int group0, int level, int64_t chunk,
                unsigned long long* __restrict__ hist, const os_state* __restrict__ state, int32_t* __restrict__ d_nan)
{
    using K = mmx_key<T>;
    using key_t = typename K::type;
    constexpr int VE = os_vec<T>::n;
    constexpr int WB = os_wbits<VE>::n;
    __shared__ uint32_t lds[kWaves][kRanks * kBins];

    const int g = group0 + (int)blockIdx.y;
    const mmx_rank_group gr = groups[g];
    const int64_t n = (int64_t)(gr.z1 - gr.z0) * ny * nx;
    const int64_t e0 = (int64_t)blockIdx.x * chunk;
    if (e0 >= n) return;                                       // (uniform: the grid is sized for the largest group)
    const int64_t cnt = n - e0 < chunk ? n - e0 : chunk;
    const os_state st = state[g];
    const int n_uniq = st.n_uniq;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t* wh = lds[wave];
    for (int i = lane; i < n_uniq * kBins; i += 64) wh[i] = 0;
    // (a wave only ever touches its own histogram until the barrier below: no barrier needed here)

    const int shift = 8 * (K::levels - 1 - level);
    const key_t up0 = (key_t)st.uprefix[0], up1 = (key_t)st.uprefix[1], up2 = (key_t)st.uprefix[2],
                up3 = (key_t)st.uprefix[3];
    bool nan = false;
    auto entry = [&](T v) {
        const key_t k = K::make(v, nan);
        const int bin = (int)((k >> shift) & 0xff);
        if (L0) return bin;
        const key_t hi = (key_t)(k >> (shift + 8));
        return hi == up0 ? bin : hi == up1 ? kBins + bin : hi == up2 ? 2 * kBins + bin
               : hi == up3 ? 3 * kBins + bin : -1;
    };
    auto one = [&](T v) { os_fold<1, 2>(wh, entry(v), 1, lane); };

    if (contiguous) {
        const T* p = vol + (int64_t)gr.z0 * sz + e0;
        // head up to the first 16-byte boundary, whole 16-byte loads, tail
        const int64_t mis = (int64_t)((16 - ((uintptr_t)p & 15)) & 15) / (int64_t)sizeof(T);
        const int64_t head = mis < cnt ? mis : cnt;
        const int64_t n_vec = (cnt - head) / VE;
        const int64_t tail0 = head + n_vec * VE;
        if (tid < head) one(p[tid]);
        const uint4* vp = reinterpret_cast<const uint4*>(p + head);
        for (int64_t v0 = 0; v0 < n_vec; v0 += 4 * MMX_WG) {
            uint4 q[4];
            bool ok[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t v = v0 + u * MMX_WG + tid;
                ok[u] = v < n_vec;
                if (ok[u]) q[u] = vp[v];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (ok[u]) {
                    int id[VE];
#pragma unroll
                    for (int j = 0; j < VE; ++j) id[j] = entry(os_elem<T>(q[u], j));
                    // what the wave is looking at: how many lanes share the first entry of the first lane that has one
                    const int a = id[0];
                    const unsigned long long act = __ballot(a >= 0);
                    bool wide = false;
                    if (act != 0) {                                        // (uniform)
                        const int first = __builtin_amdgcn_readlane(a, (int)__ffsll((long long)act) - 1);
                        wide = (int)__popcll(__ballot(a == first)) < kFoldMin;
                    }
                    if (wide) {
                        // a wide histogram (the low bytes of noisy voxels): folding only costs, and the atomics spread
                        // over many bins anyway
#pragma unroll
                        for (int j = 0; j < VE; ++j) os_add(wh, id[j]);
                    } else {
                        // a narrow one: every lane first gathers its own elements -- the first entry and the first
                        // one that differs from it, each with its count --, then the wave folds those two per lane
                        int ca = 1, b = -1;
#pragma unroll
                        for (int j = 1; j < VE; ++j) {
                            ca += id[j] == a;
                            b = (b < 0 && id[j] != a) ? id[j] : b;
                        }
                        os_fold<WB, 2>(wh, a, ca, lane);
                        if (__ballot(b >= 0) != 0) {                       // (uniform)
                            int cb = 0;
                            bool more = false;
#pragma unroll
                            for (int j = 1; j < VE; ++j) {
                                cb += id[j] == b;
                                more = more || (id[j] >= 0 && id[j] != a && id[j] != b);
                            }
                            os_fold<WB, 2>(wh, b, cb, lane);
                            if (__ballot(more) != 0) {                     // (uniform) a third value in some lane:
                                // folded while the lanes that have one agree (an image of few values), else (the
                                // bright tail of a plane, spread over many bins) straight to the atomics
                                bool agree = true;
#pragma unroll
                                for (int j = 2; j < VE; ++j) {
                                    const int e = (id[j] != a && id[j] != b) ? id[j] : -1;
                                    if (agree) agree = os_fold<1, 1>(wh, e, 1, lane) >= kFoldMin;
                                    else os_add(wh, e);
                                }
                            }
                        }
                    }
                }
            }
        }
        if (tail0 + tid < cnt) one(p[tail0 + tid]);
    } else {
        const int64_t plane = ny * nx;
        for (int64_t i = tid; i < cnt; i += MMX_WG) {
            const int64_t e = e0 + i;
            const int64_t z = e / plane, r = e - z * plane;
            const int64_t y = r / nx, x = r - y * nx;
            one(vol[((int64_t)gr.z0 + z) * sz + y * sy + x * sx]);
        }
    }
    if (L0 && nan) d_nan[g] = 1;
    __syncthreads();
    unsigned long long* gh = hist + (int64_t)g * kRanks * kBins;
    for (int i = tid; i < n_uniq * kBins; i += MMX_WG) {
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) c += lds[w][i];
        if (c) atomicAdd(&gh[i], (unsigned long long)c);
    }
}

// the levels' state before the first pass: no byte chosen, every rank on histogram 0
__global__ void __launch_bounds__(MMX_WG)
os_init_kernel(const mmx_rank_group* __restrict__ groups, int n_groups, os_state* __restrict__ state)
{
    const int g = (int)blockIdx.x * MMX_WG + (int)threadIdx.x;
    if (g >= n_groups) return;
    os_state st;
    for (int r = 0; r < kRanks; ++r) {
        st.prefix[r] = 0;
        st.rem[r] = (unsigned long long)groups[g].rank[r];
        st.uprefix[r] = r == 0 ? 0ull : ~0ull;
        st.slot[r] = 0;
    }
    st.n_uniq = 1;
    st._pad[0] = st._pad[1] = st._pad[2] = 0;
    state[g] = st;
}

template <typename T>
__global__ void __launch_bounds__(MMX_WG)
os_select_kernel(unsigned long long* __restrict__ hist, os_state* __restrict__ state, int last,
                 double* __restrict__ d_stats)
{
    static_assert(kWaves == kRanks, "one wave per rank");
    __shared__ unsigned long long s_prefix[kRanks], s_rem[kRanks];
    __shared__ int s_slot[kRanks];
    const int g = (int)blockIdx.x;
    const int tid = (int)threadIdx.x, lane = tid & 63, r = tid >> 6;
    unsigned long long* gh = hist + (int64_t)g * kRanks * kBins;
    os_state* st = state + g;
    const int n_uniq_now = st->n_uniq;
    {
        const unsigned long long* h = gh + st->slot[r] * kBins + 4 * lane;
        const unsigned long long c0 = h[0], c1 = h[1], c2 = h[2], c3 = h[3];
        const unsigned long long mine = c0 + c1 + c2 + c3;
        unsigned long long incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        unsigned long long below = incl - mine;
        const unsigned long long rem = st->rem[r];
        if (below <= rem && rem < incl) {                      // exactly one lane: the bins sum to more than rem
            int b = 4 * lane;
            if (rem >= below + c0) { below += c0; ++b;
                if (rem >= below + c1) { below += c1; ++b;
                    if (rem >= below + c2) { below += c2; ++b; } } }
            s_prefix[r] = (st->prefix[r] << 8) | (unsigned long long)b;
            s_rem[r] = rem - below;
        }
    }
    __syncthreads();                                           // (every read of the state and the bins is behind us)
    for (int i = tid; i < n_uniq_now * kBins; i += MMX_WG) gh[i] = 0;
    if (last) {
        if (tid < kRanks) d_stats[(int64_t)g * kRanks + tid] = mmx_key<T>::value(s_prefix[tid]);
    } else if (tid == 0) {
        int n_uniq = 0;
        for (int k = 0; k < kRanks; ++k) {
            st->prefix[k] = s_prefix[k];
            st->rem[k] = s_rem[k];
            st->uprefix[k] = ~0ull;
        }
        for (int k = 0; k < kRanks; ++k) {
            int s = -1;
            for (int j = 0; j < k; ++j)
                if (s < 0 && s_prefix[j] == s_prefix[k]) s = s_slot[j];
            if (s < 0) { s = n_uniq++; st->uprefix[s] = s_prefix[k]; }
            s_slot[k] = s;
            st->slot[k] = s;
        }
        st->n_uniq = n_uniq;
    }
}

int64_t os_align(int64_t v) { return (v + 255) & ~int64_t(255); }

template <typename T>
int os_run(const mmx_volume* vol, int64_t ny, int64_t nx, const mmx_rank_group* d_groups, int n_groups,
           int64_t max_voxels, double* d_stats, int32_t* d_nan, unsigned long long* hist, os_state* state, hipStream_t s)
{
    const int contiguous = vol->stride_x == 1 && vol->stride_y == nx && vol->stride_z == ny * nx;
    const int64_t chunk = contiguous ? kChunkBytes / (int64_t)sizeof(T) : kChunkStrided;
    const int64_t chunks = (max_voxels + chunk - 1) / chunk;
    if (chunks > MMX_MAX_GRID_X) return MMX_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(os_init_kernel, dim3((unsigned)((n_groups + MMX_WG - 1) / MMX_WG)), dim3(MMX_WG), 0, s,
                       d_groups, n_groups, state);
    for (int level = 0; level < mmx_key<T>::levels; ++level) {
        for (int g0 = 0; g0 < n_groups; g0 += MMX_MAX_BLOCKS) {
            const int ng = std::min(MMX_MAX_BLOCKS, n_groups - g0);
            auto count = level == 0 ? os_count_kernel<T, true> : os_count_kernel<T, false>;
            hipLaunchKernelGGL(count, dim3((unsigned)chunks, (unsigned)ng), dim3(MMX_WG), 0, s,
                               (const T*)vol->d_data, vol->stride_z, vol->stride_y, vol->stride_x, ny, nx, contiguous,
                               d_groups, g0, level, chunk, hist, (const os_state*)state, d_nan);
        }
        hipLaunchKernelGGL(os_select_kernel<T>, dim3((unsigned)n_groups), dim3(MMX_WG), 0, s, hist, state,
                           level == mmx_key<T>::levels - 1 ? 1 : 0, d_stats);
    }
    return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
}

}  // namespace

extern "C" size_t mmx_order_stats_workspace(int n_groups)
{
    if (n_groups < 1) return 0;
    return (size_t)(os_align((int64_t)n_groups * kRanks * kBins * (int64_t)sizeof(unsigned long long)) +
                    os_align((int64_t)n_groups * (int64_t)sizeof(os_state)));
}

extern "C" int mmx_order_stats(const mmx_volume* vol, int64_t nz, int64_t ny, int64_t nx,
                               const mmx_rank_group* d_groups, const mmx_rank_group* h_groups, int n_groups,
                               double* d_stats, int32_t* d_nan, void* d_work, size_t work_bytes, void* stream)
{
    if (!vol || !vol->d_data || !d_groups || !h_groups || n_groups < 1 || !d_stats || !d_nan || !d_work)
        return MMX_ERR_ARG;
    if (nz < 1 || ny < 1 || nx < 1 || nz > 0x7fffffff || ny > 0x7fffffff || nx > 0x7fffffff) return MMX_ERR_ARG;
    if (!mmx_voxel_in(vol->dtype, MMX_VOX_ALL)) return MMX_ERR_ARG;      // (ahead of the memsets: a refusal writes nothing)
    if (((uintptr_t)d_work & 15) != 0) return MMX_ERR_ARG;
    int64_t max_voxels = 0;
    for (int g = 0; g < n_groups; ++g) {
        const mmx_rank_group& gr = h_groups[g];
        if (gr.z0 < 0 || gr.z1 <= gr.z0 || gr.z1 > nz) return MMX_ERR_ARG;
        const int64_t n = (int64_t)(gr.z1 - gr.z0) * ny * nx;
        for (int r = 0; r < kRanks; ++r)
            if (gr.rank[r] < 0 || gr.rank[r] >= n) return MMX_ERR_ARG;
        max_voxels = std::max(max_voxels, n);
    }
    if (work_bytes < mmx_order_stats_workspace(n_groups)) return MMX_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t hist_bytes = os_align((int64_t)n_groups * kRanks * kBins * (int64_t)sizeof(unsigned long long));
    unsigned long long* hist = (unsigned long long*)d_work;
    os_state* state = (os_state*)((char*)d_work + hist_bytes);
    if (hipMemsetAsync(hist, 0, (size_t)hist_bytes, s) != hipSuccess) return MMX_ERR_HIP;
    if (hipMemsetAsync(d_nan, 0, (size_t)n_groups * sizeof(int32_t), s) != hipSuccess) return MMX_ERR_HIP;
    return mmx_for_voxel<MMX_VOX_ALL>(vol->dtype, MMX_ERR_ARG, [&](auto t) {
        return os_run<MMX_TAG_T(t)>(vol, ny, nx, d_groups, n_groups, max_voxels, d_stats, d_nan, hist, state, s);
    });
}
