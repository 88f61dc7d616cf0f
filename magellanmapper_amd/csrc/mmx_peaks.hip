// Scale-space local maxima (A4): 3x3x3x3 non-max suppression over (z, y, x, sigma).
//
// Replaces skimage.feature.peak_local_max as blob_log calls it
// (skimage/feature/blob.py:506-512 -> skimage/feature/peak.py:28-50, 114-319):
//   mask = (cube == maximum_filter(cube, footprint=ones(3,3,3,3), mode='constant'))
//          & (cube > threshold)
// i.e. a voxel is a peak when it is >= its 80 neighbours (0 outside the cube, also past
// the first / last sigma) and strictly above the threshold.
//
// The float32 cube cannot decide exact ties, so this kernel emits CANDIDATES: voxels with
// v >= nbr_max - eps and v > thr - eps, flagged "contested" unless they win by more than
// eps on both tests.  Exact float64 values (mmx_rescore.hip) settle the rest on the host.
//
// Design (gfx950): one coalesced read of each sigma plane per voxel (the algorithmic
// 4 B/voxel/sigma); almost every voxel fails `v > thr - eps` and stops there.  The 80
// neighbour reads happen only inside blobs and come from L1/L2.  Hits are appended with
// a wave-aggregated atomic counter.

#include "mmx_common.h"

namespace {

constexpr int kSigmaChunk = 8;   // sigma planes whose loads are issued back to back

struct peak_ctx {
    const float* base;      // slot base of sigma 0
    int64_t sigma_stride;
    int ns, nz, ny, nx, px, plane, slot;
    float thr, eps;
    mmx_cand* out;
    uint32_t cap;
    uint32_t* count;
};

// Full 80-neighbour test of one voxel that passed `v > thr - eps` (rare: inside blobs only).
__device__ __forceinline__ void check_voxel(const peak_ctx& c, int s, int idx, float v)
{
    const int z = idx / c.plane;
    const int rem = idx - z * c.plane;
    const int y = rem / c.px;
    const int x = rem - y * c.px;
    const int nz = c.nz, ny = c.ny, nx = c.nx, px = c.px, plane = c.plane;
    const float reject = v + c.eps;  // a neighbour above this rules the voxel out
    float m = -INFINITY;
    bool border = false;
    // same-sigma face neighbours first: they reject nearly every non-peak
    const float* ps = c.base + (int64_t)s * c.sigma_stride;
    if (x > 0) m = fmaxf(m, ps[idx - 1]); else border = true;
    if (x + 1 < nx) m = fmaxf(m, ps[idx + 1]); else border = true;
    if (y > 0) m = fmaxf(m, ps[idx - px]); else border = true;
    if (y + 1 < ny) m = fmaxf(m, ps[idx + px]); else border = true;
    if (z > 0) m = fmaxf(m, ps[idx - plane]); else border = true;
    if (z + 1 < nz) m = fmaxf(m, ps[idx + plane]); else border = true;
    if (m > reject) return;
    for (int ds = -1; ds <= 1; ++ds) {
        const int ss = s + ds;
        if (ss < 0 || ss >= c.ns) { border = true; continue; }
        const float* pss = c.base + (int64_t)ss * c.sigma_stride;
        for (int dz = -1; dz <= 1; ++dz) {
            const int zz = z + dz;
            if (zz < 0 || zz >= nz) continue;  // border already noted above
            for (int dy = -1; dy <= 1; ++dy) {
                const int yy = y + dy;
                if (yy < 0 || yy >= ny) continue;
                const int row = zz * plane + yy * px;
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int xx = x + dx;
                    if (xx < 0 || xx >= nx) continue;
                    if ((ds | dz | dy | dx) == 0) continue;
                    m = fmaxf(m, pss[row + xx]);
                }
            }
            if (m > reject) return;
        }
    }
    if (border) m = fmaxf(m, 0.0f);  // mode='constant', cval = 0
    if (!(v >= m - c.eps)) return;
    const bool contested = !(v > m + c.eps) || !(v > c.thr + c.eps);
    const uint32_t pos = atomicAdd(c.count, 1u);
    if (pos < c.cap) {
        mmx_cand r;
        r.slot = c.slot;
        r.s = s;
        r.z = z;
        r.y = y;
        r.x = x;
        r.flags = contested ? MMX_CAND_CONTESTED : 0u;
        r.v = v;
        r.nbr_max = m;
        r.v64 = __longlong_as_double(0x7ff8000000000000LL);
        r.band = 0;
        c.out[pos] = r;
    }
}

// Thread = 4 consecutive x (one 16-byte load per sigma plane; rows are 128-B aligned), all
// sigma loads of a chunk issued before any is tested.
__global__ void __launch_bounds__(MMX_WG)
peaks_kernel(const float* __restrict__ log, int ns, int64_t sigma_stride,
             const mmx_block* __restrict__ blocks, int64_t slot_elems, float thr, float eps,
             mmx_cand* __restrict__ out, uint32_t cap, uint32_t* __restrict__ count)
{
    const mmx_block bd = blocks[blockIdx.y];
    peak_ctx c;
    c.base = log + (int64_t)bd.slot * slot_elems;
    c.sigma_stride = sigma_stride;
    c.ns = ns; c.nz = bd.nz; c.ny = bd.ny; c.nx = bd.nx; c.px = bd.px;
    c.plane = bd.ny * bd.px; c.slot = bd.slot;
    c.thr = thr; c.eps = eps; c.out = out; c.cap = cap; c.count = count;
    const int nquads = bd.nz * c.plane / 4;
    const float lo = thr - eps;
    const int qrow = bd.px / 4;          // quads per row

    for (int q = blockIdx.x * MMX_WG + threadIdx.x; q < nquads; q += gridDim.x * MMX_WG) {
        const int x0 = (q % qrow) * 4;
        if (x0 >= bd.nx) continue;       // pitch columns
        const float4* p = reinterpret_cast<const float4*>(c.base) + q;
        const int64_t sstride4 = sigma_stride / 4;
        const int lane = threadIdx.x & 63;
        const bool has_left = x0 > 0 && lane > 0;            // lane - 1 holds x0-4 .. x0-1 of this row
        const bool has_right = x0 + 4 < bd.nx && lane < 63 && q + 1 < nquads;  // lane + 1: x0+4 .. x0+7
        const bool ok1 = x0 + 1 < bd.nx, ok2 = x0 + 2 < bd.nx, ok3 = x0 + 3 < bd.nx;
        for (int s0 = 0; s0 < ns; s0 += kSigmaChunk) {
            // e?[k + 1] = element ? of sigma s0 + k; index 0 and kSigmaChunk + 1 are the neighbouring
            // scales (-inf outside the ladder: zero padding can never out-vote a value > thr >= 0).
            // Plain scalar arrays with compile-time indices only: they must stay in registers.
            float e0[kSigmaChunk + 2], e1[kSigmaChunk + 2], e2[kSigmaChunk + 2], e3[kSigmaChunk + 2];
#pragma unroll
            for (int k = 0; k < kSigmaChunk + 2; ++k) {
                const int s = s0 + k - 1;
                float4 v = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
                if (s >= 0 && s < ns) v = p[(int64_t)s * sstride4];
                // pitch columns hold no data: they must never out-vote a real neighbour
                e0[k] = v.x;
                e1[k] = ok1 ? v.y : -INFINITY;
                e2[k] = ok2 ? v.z : -INFINITY;
                e3[k] = ok3 ? v.w : -INFINITY;
            }
            // In-register pre-filter: a 4-D local maximum must beat its two x neighbours and the
            // same voxel one scale up / down (all already in registers or one lane away).  Only
            // survivors pay for the remaining 76 neighbour reads.
            unsigned hits = 0;
#pragma unroll
            for (int k = 1; k <= kSigmaChunk; ++k) {
                if (s0 + k - 1 < ns) {
                    float lft = __shfl_up(e3[k], 1);
                    float rgt = __shfl_down(e0[k], 1);
                    lft = has_left ? lft : -INFINITY;
                    rgt = has_right ? rgt : -INFINITY;
                    const float n0 = fmaxf(fmaxf(lft, e1[k]), fmaxf(e0[k - 1], e0[k + 1]));
                    const float n1 = fmaxf(fmaxf(e0[k], e2[k]), fmaxf(e1[k - 1], e1[k + 1]));
                    const float n2 = fmaxf(fmaxf(e1[k], e3[k]), fmaxf(e2[k - 1], e2[k + 1]));
                    const float n3 = fmaxf(fmaxf(e2[k], rgt), fmaxf(e3[k - 1], e3[k + 1]));
                    const unsigned sh = 4 * (k - 1);
                    hits |= (mmx_candidate(true, e0[k], lo, eps, n0) ? 1u : 0u) << sh;
                    hits |= (mmx_candidate(true, e1[k], lo, eps, n1) ? 2u : 0u) << sh;
                    hits |= (mmx_candidate(true, e2[k], lo, eps, n2) ? 4u : 0u) << sh;
                    hits |= (mmx_candidate(true, e3[k], lo, eps, n3) ? 8u : 0u) << sh;
                }
            }
            while (hits) {              // rare: only inside blobs
                const int b = __ffs(hits) - 1;
                hits &= hits - 1;
                const int j = b & 3;
                if (x0 + j >= bd.nx) continue;
                const int s = s0 + (b >> 2);
                const int idx = 4 * q + j;
                check_voxel(c, s, idx, c.base[(int64_t)s * sigma_stride + idx]);
            }
        }
    }
}

// ---- sparse variant: works from the entries the Y pass of the fused and wide paths leaves (mmx_entries.h):
// .x = candidate bits, .y = "above thr - eps" bits.  Segments with .y == 0 were not stored: their voxels count as
// -inf (they can neither be peaks nor out-vote a candidate, which is above thr - eps itself).
struct sparse_ctx {
    peak_ctx c;
    const ulonglong2* ent;      // entries of this block, sigma 0
    int64_t ent_sigma_stride;   // entries per sigma
    mmx_entry_geom eg;          // the layout
};

// entry holding voxel (z, y, x)
__device__ __forceinline__ int64_t sparse_entry(const sparse_ctx& k, int z, int y, int x)
{
    return (int64_t)y * k.eg.per_row + mmx_entry_index(k.eg, z, x);
}

__device__ __forceinline__ float sparse_at(const sparse_ctx& k, int s, int z, int y, int x)
{
    const unsigned long long above = k.ent[(int64_t)s * k.ent_sigma_stride + sparse_entry(k, z, y, x)].y;
    if (!above) return -INFINITY;
    return k.c.base[(int64_t)s * k.c.sigma_stride + (int64_t)z * k.c.plane + y * k.c.px + x];
}

// One group of 32 lanes tests one voxel that passed the pre-check against all 80 neighbours: lane l < 27 takes the row
// (ds, dz, dy) = (l / 9 - 1, l / 3 % 3 - 1, l % 3 - 1), loads its (at most two) entries with the centre's value, then
// its three values, all addresses clamped into the cube and every value load of a neighbour that is outside, the centre
// or unstored pointed at the centre instead (a voxel that is certainly stored) -- two memory round trips per voxel.  The
// group then reduces the maximum and the 80 band bits, and its first lane applies the rule and appends the row.
// Same decisions as check_voxel on the stored cube: a neighbour that is not stored is below thr - eps < v.
__device__ __forceinline__ void check_voxel_sparse_group(const sparse_ctx& k, int s, int z, int y, int x, int l)
{
    const peak_ctx& c = k.c;
    const int nz = c.nz, ny = c.ny, nx = c.nx;
    const int ds = l / 9 - 1, dz = (l / 3) % 3 - 1, dy = l % 3 - 1;
    const int ss = s + ds, zz = z + dz, yy = y + dy;
    const bool row_ok = l < 27 && ss >= 0 && ss < c.ns && zz >= 0 && zz < nz && yy >= 0 && yy < ny;
    const int sc = min(max(ss, 0), c.ns - 1), zc = min(max(zz, 0), nz - 1), yc = min(max(yy, 0), ny - 1);
    const int xl = max(x - 1, 0), xr = min(x + 1, nx - 1);
    const float* ctr = c.base + (int64_t)s * c.sigma_stride + (int64_t)z * c.plane + y * c.px + x;
    const ulonglong2* er = k.ent + (int64_t)sc * k.ent_sigma_stride + (int64_t)yc * k.eg.per_row;
    // the three x neighbours share at most two entries: the middle one lies in its left or its right neighbour's
    const int el = mmx_entry_index(k.eg, zc, xl), em = mmx_entry_index(k.eg, zc, x), er_i = mmx_entry_index(k.eg, zc, xr);
    const float v = *ctr;
    const unsigned long long al = er[el].y;
    const unsigned long long ar = er[er_i].y;
    const unsigned long long am = em == el ? al : ar;
    const float* row = c.base + (int64_t)sc * c.sigma_stride + (int64_t)zc * c.plane + yc * c.px;
    const bool ok0 = row_ok && x > 0 && al != 0;
    const bool ok1 = row_ok && l != 13 && am != 0;
    const bool ok2 = row_ok && x + 1 < nx && ar != 0;
    const float r0 = *(ok0 ? row + x - 1 : ctr);
    const float r1 = *(ok1 ? row + x : ctr);
    const float r2 = *(ok2 ? row + x + 1 : ctr);
    const float u0 = ok0 ? r0 : -INFINITY, u1 = ok1 ? r1 : -INFINITY, u2 = ok2 ? r2 : -INFINITY;
    float m = fmaxf(fmaxf(u0, u1), u2);
    // which of the 80 neighbours (C order of (ds, dz, dy, dx), the centre left out) lie in the band: the only ones
    // whose exact values the host needs when the candidate turns out contested
    const float band_lo = v - c.eps;       // a neighbour below this cannot out-vote the candidate whatever the exact values
    unsigned b_lo = 0, b_mid = 0, b_hi = 0;     // bits 0..31, 32..63, 64..79
    auto mark = [&](bool in, int j) __attribute__((always_inline)) {
        j -= j > 40;
        const unsigned bit = in ? 1u << (j & 31) : 0u;
        if (j < 32) b_lo |= bit; else if (j < 64) b_mid |= bit; else b_hi |= bit;
    };
    mark(u0 >= band_lo, 3 * l);
    mark(u1 >= band_lo, 3 * l + 1);
    mark(u2 >= band_lo, 3 * l + 2);
#pragma unroll
    for (int d = 16; d >= 1; d >>= 1) {
        m = fmaxf(m, __shfl_xor(m, d, 32));
        b_lo |= (unsigned)__shfl_xor((int)b_lo, d, 32);
        b_mid |= (unsigned)__shfl_xor((int)b_mid, d, 32);
        b_hi |= (unsigned)__shfl_xor((int)b_hi, d, 32);
    }
    if (l != 0) return;
    if (m > v + c.eps) return;              // a neighbour above this rules the voxel out
    const bool border = s == 0 || s + 1 == c.ns || z == 0 || z + 1 == nz || y == 0 || y + 1 == ny || x == 0 || x + 1 == nx;
    if (border) m = fmaxf(m, 0.0f);  // mode='constant', cval = 0
    if (!(v >= m - c.eps)) return;
    const bool contested = !(v > m + c.eps) || !(v > c.thr + c.eps);
    const uint32_t pos = atomicAdd(c.count, 1u);
    if (pos < c.cap) {
        mmx_cand r;
        r.slot = c.slot;
        r.s = s;
        r.z = z;
        r.y = y;
        r.x = x;
        r.flags = (contested ? MMX_CAND_CONTESTED : 0u) | MMX_CAND_BAND | (b_hi << 16);
        r.v = v;
        r.nbr_max = m;
        r.v64 = __longlong_as_double(0x7ff8000000000000LL);
        r.band = ((unsigned long long)b_mid << 32) | b_lo;
        c.out[pos] = r;
    }
}

// One lane per entry and sigma: nearly all candidate words are zero.  The workgroup queues the set bits of its 2048
// words in LDS and works the queue off in two stages, each with its loads in flight together instead of in a chain:
//   1. one lane per queued bit: the voxel against z +- 1 and sigma +- 1 (the y and x neighbours were tested when the bit
//      was set: most set bits are the in-plane maxima of the z-slices and scales of a blob and fall here) -- its value
//      and the four entries in one round trip, the four values in a second;
//   2. the few per cent that survive, queued again: a group of 32 lanes per voxel (check_voxel_sparse_group).
// Either queue is worked off whenever it could not take what comes next, so a dense patch costs rounds, not correctness.
__global__ void __launch_bounds__(MMX_WG)
peaks_sparse_kernel(const float* __restrict__ log, const ulonglong2* __restrict__ entries,
                    int ns, int64_t sigma_stride, const mmx_block* __restrict__ blocks, int64_t slot_elems,
                    float thr, float eps, mmx_cand* __restrict__ out, uint32_t cap,
                    uint32_t* __restrict__ count, int quads)
{
    const mmx_block bd = blocks[blockIdx.y];
    sparse_ctx k;
    peak_ctx& c = k.c;
    c.base = log + (int64_t)bd.slot * slot_elems;
    c.sigma_stride = sigma_stride;
    c.ns = ns; c.nz = bd.nz; c.ny = bd.ny; c.nx = bd.nx; c.px = bd.px;
    c.plane = bd.ny * bd.px; c.slot = bd.slot;
    c.thr = thr; c.eps = eps; c.out = out; c.cap = cap; c.count = count;
    k.eg = mmx_entry_geom_make(quads ? MMX_MASK_QUADS : MMX_MASK_ROWS, bd.nz, bd.nx, bd.px);
    k.ent = entries + mmx_entry_base(bd.slot, slot_elems);
    k.ent_sigma_stride = sigma_stride >> 5;
    const int64_t per_sigma = (int64_t)bd.ny * k.eg.per_row;
    const int64_t total = per_sigma * ns;
    constexpr int kQ = 1024;                // queued bits: (word index << 6) | bit
    constexpr int kQ2 = 512;                // survivors of stage 1, the same items
    __shared__ unsigned long long q[kQ];
    __shared__ unsigned long long q2[kQ2];
    __shared__ int qn, q2n;
    // word index and bit -> the voxel; false: a bit of a pitch column or of a plane past the block
    auto voxel_of = [&](unsigned long long e, int* s, int* z, int* y, int* x) __attribute__((always_inline)) -> bool {
        const int64_t i = (int64_t)(e >> 6);
        *s = (int)(i / per_sigma);
        const int64_t r = i - (int64_t)*s * per_sigma;
        *y = (int)(r / k.eg.per_row);
        const int w = (int)(r - (int64_t)*y * k.eg.per_row);
        mmx_entry_voxel(k.eg, w, (int)(e & 63), z, x);
        return *x < bd.nx && *z < bd.nz;
    };
    // stage 1 on one queued item: true when the voxel goes on to stage 2
    auto pre_check = [&](unsigned long long e) __attribute__((always_inline)) -> bool {
        int s, z, y, x;
        const bool real = voxel_of(e, &s, &z, &y, &x);
        z = min(z, bd.nz - 1);              // (an item that is no voxel still loads inside the cube)
        x = min(x, bd.nx - 1);
        const float* ctr = c.base + (int64_t)s * sigma_stride + (int64_t)z * c.plane + y * bd.px + x;
        const int zd = max(z - 1, 0), zu = min(z + 1, bd.nz - 1), sd = max(s - 1, 0), su = min(s + 1, ns - 1);
        const ulonglong2* ey = k.ent + (int64_t)y * k.eg.per_row;
        const int64_t es = (int64_t)s * k.ent_sigma_stride;
        const int ec = mmx_entry_index(k.eg, z, x);
        const float v = *ctr;
        const unsigned long long a0 = ey[es + mmx_entry_index(k.eg, zd, x)].y;
        const unsigned long long a1 = ey[es + mmx_entry_index(k.eg, zu, x)].y;
        const unsigned long long a2 = ey[(int64_t)sd * k.ent_sigma_stride + ec].y;
        const unsigned long long a3 = ey[(int64_t)su * k.ent_sigma_stride + ec].y;
        const bool ok0 = z > 0 && a0 != 0, ok1 = z + 1 < bd.nz && a1 != 0, ok2 = s > 0 && a2 != 0, ok3 = s + 1 < ns && a3 != 0;
        const float r0 = *(ok0 ? ctr - c.plane : ctr);
        const float r1 = *(ok1 ? ctr + c.plane : ctr);
        const float r2 = *(ok2 ? ctr - sigma_stride : ctr);
        const float r3 = *(ok3 ? ctr + sigma_stride : ctr);
        const float n0 = ok0 ? r0 : -INFINITY, n1 = ok1 ? r1 : -INFINITY, n2 = ok2 ? r2 : -INFINITY, n3 = ok3 ? r3 : -INFINITY;
        return real && !(fmaxf(fmaxf(n0, n1), fmaxf(n2, n3)) > v + eps);
    };
    // stage 2 on the survivors queued so far (every lane of the workgroup calls it)
    auto full_test = [&]() __attribute__((always_inline)) {
        __syncthreads();
        const int n2 = q2n;
        const int l = threadIdx.x & 31;
        for (int t = threadIdx.x >> 5; t < n2; t += MMX_WG / 32) {
            int s, z, y, x;
            voxel_of(q2[t], &s, &z, &y, &x);
            check_voxel_sparse_group(k, s, z, y, x, l);
        }
        __syncthreads();
        if (threadIdx.x == 0) q2n = 0;
    };
    if (threadIdx.x == 0) { qn = 0; q2n = 0; }
    __syncthreads();
    constexpr int kW = 8;                          // words per lane and round
    const int64_t stride = (int64_t)gridDim.x * MMX_WG * kW;
    const int64_t rounds = (total + stride - 1) / stride;
    for (int64_t rd = 0; rd < rounds; ++rd) {
        const int64_t i0 = rd * stride + (int64_t)blockIdx.x * MMX_WG * kW + threadIdx.x;
        unsigned long long mw[kW];
#pragma unroll
        for (int u = 0; u < kW; ++u) {
            const int64_t i = i0 + (int64_t)u * MMX_WG;
            mw[u] = 0;
            if (i < total) {
                const int s = (int)(i / per_sigma);
                mw[u] = k.ent[(int64_t)s * k.ent_sigma_stride + (i - (int64_t)s * per_sigma)].x;
            }
        }
        // Set bits are rare (a few per cent of the words hold one).  A dense patch holds more than the queue: a lane
        // queues what fits, keeps the rest of its words, and the workgroup goes round again once the queue is empty.
        for (;;) {
            bool left = false;                    // this lane still holds bits
#pragma unroll
            for (int u = 0; u < kW; ++u) {
                unsigned long long m = mw[u];
                if (!m || left) { left = left || m != 0; continue; }
                const int64_t i = i0 + (int64_t)u * MMX_WG;
                const int cnt = __popcll(m);
                const int at = atomicAdd(&qn, cnt);
                int fit = kQ - at;                // (slots at .. kQ - 1 are this lane's, whatever else was asked for)
                fit = fit < 0 ? 0 : fit < cnt ? fit : cnt;
                for (int j = at; j < at + fit; ++j) {
                    const int b = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    q[j] = ((unsigned long long)i << 6) | (unsigned long long)b;
                }
                mw[u] = m;
                left = m != 0;
            }
            __syncthreads();
            const int nq = qn < kQ ? qn : kQ;     // (the queue is dense: every slot below nq was written)
            for (int j0 = 0; j0 < nq; j0 += MMX_WG) {
                const int j = j0 + threadIdx.x;
                const unsigned long long e = j < nq ? q[j] : 0;
                if (j < nq && pre_check(e)) q2[atomicAdd(&q2n, 1)] = e;
                // (at most 256 survivors a pass: stage 2 runs once the next pass might not fit, and at the end)
                if (j0 + MMX_WG < nq) {
                    __syncthreads();
                    if (q2n > kQ2 - MMX_WG) full_test();
                    __syncthreads();
                }
            }
            full_test();
            if (threadIdx.x == 0) qn = 0;
            if (!__syncthreads_or(left)) break;
        }
    }
}

}  // namespace

int mmx_launch_peaks_sparse(const float* d_log, const unsigned long long* d_mask, int n_sigma,
                            int64_t sigma_stride, const mmx_block* d_blocks, int n_blocks, int max_vox,
                            int64_t slot_elems, float thr, float eps, mmx_cand* d_cands, uint32_t cap,
                            uint32_t* d_count, int quads, hipStream_t stream)
{
    int64_t words = ((int64_t)max_vox / 64 + 1024) * n_sigma;
    int gx = (int)((words + MMX_WG * 8 - 1) / (MMX_WG * 8));      // 8 words per lane and round
    if (gx > 8192) gx = 8192;
    if (gx < 1) gx = 1;
    dim3 grid(gx, n_blocks);
    hipLaunchKernelGGL(peaks_sparse_kernel, grid, dim3(MMX_WG), 0, stream, d_log,
                       reinterpret_cast<const ulonglong2*>(d_mask), n_sigma, sigma_stride,
                       d_blocks, slot_elems, thr, eps, d_cands, cap, d_count, quads);
    return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
}

int mmx_launch_peaks(const float* d_log, int n_sigma, int64_t sigma_stride, const mmx_block* d_blocks,
                     int n_blocks, int max_vox, int64_t slot_elems, float thr, float eps,
                     mmx_cand* d_cands, uint32_t cap, uint32_t* d_count, hipStream_t stream)
{
    int gx = (max_vox / 4 + MMX_WG - 1) / MMX_WG;
    if (gx > 8192) gx = 8192;
    if (gx < 1) gx = 1;
    dim3 grid(gx, n_blocks);
    hipLaunchKernelGGL(peaks_kernel, grid, dim3(MMX_WG), 0, stream, d_log, n_sigma, sigma_stride,
                       d_blocks, slot_elems, thr, eps, d_cands, cap, d_count);
    return hipGetLastError() == hipSuccess ? MMX_OK : MMX_ERR_HIP;
}
