// The per-tile statistics and element-wise rules of the preprocessing, stated once for every kernel form
// (mmx_preproc.hip: one workgroup per tile with the whole life of the tile in one kernel -- pp_fast_kernel,
// pp_mid_kernel, pp_generic_kernel; mmx_preproc_pipe.hip: pp_stats_kernel + the pipelined pp_blur_kernel).
// A kernel keeps its own voxel walk (loads in flight, LDS / scratch / buffer loads) and its own high-byte histogram;
// the stages between and after them are the helpers below, in the order a tile meets them:
//   pp_select_high -> pp_bins::add -> pp_select_low      the four order statistics np.percentile interpolates between
//   pp_key_bounds / pp_make_bounds -> pp_sat_t::make     vmin, vmax, identity -> the stretch
//   pp_mean_verdict, pp_exact_verdict                    the mean's tolerance, knife edge and erosion flag
//   pp_write_info                                        the tile's mmx_subblock_info record
//   pp_unsharp, pp_erode7, pp_put                        the unsharp mask, the 7-point minimum, both output copies
// plus the leaves they are built from (pp_select, pp_pairwise, pp_line_pass, ...).
#pragma once

#include <algorithm>

#include "mmx_common.h"

#define PP_R 32          // int(4 * 8 + 0.5): sigma 8 is hard-coded in plot_3d.py:151
#define PP_MAXL 32       // longest line of the register-resident pass
#define PP_WG 640        // 10 waves: 625 lines of a 25^3 sub-block in one round
#define PP_WG_GENERIC 1024
#define PP_HIST (5 * 256)
#define PP_NB_LOAD 13     // global loads in flight per lane (25 rows = 13 + 12)
#define PP_NB 9           // voxels in flight per lane in the arithmetic stages (25 rows = 9 + 9 + 7)

struct pp_args {
    double clip_min, clip_max, max_thresh, strength, ero_thr;
    double tv_weight, tv_factor;          // total-variation denoising: weight (0 = off), tau / weight
    int64_t dst_sy, dst_sz;
    int32_t do_unsharp, do_erosion, rgb_guess, _pad;
};
#define PP_TV_SCRATCH 7      // doubles of scratch per voxel with total-variation denoising on (2 without)
#define PP_MAXLEAF 2048      // leaves of NumPy's pairwise summation tree kept in LDS (n <= ~130 000 voxels)
#define MMX_PP_KNIFE 0x100   // internal flag: the statistics kernel asks the blur kernel for np.mean's own summation order

namespace {

__device__ __forceinline__ double pp_clip(double x, double lo, double hi)
{
    // np.clip == minimum(maximum(x, lo), hi); no NaNs on this path, so v_max_f64 / v_min_f64 agree
    return fmin(fmax(x, lo), hi);
}

// numpy _lerp (numpy/lib/_function_base_impl.py): a + (b-a)*t, or b - (b-a)*(1-t) for t >= 0.5
__device__ __forceinline__ double pp_lerp(double a, double b, double t)      // (float64 images: the same NumPy formula)
{
    const double d = b - a;
    double r = a + d * t;
    if (t >= 0.5) r = b - d * (1.0 - t);
    return r;
}
__device__ __forceinline__ double pp_lerp(int a, int b, double t)
{
    const double d = (double)(b - a);
    double r = (double)a + d * t;
    if (t >= 0.5) r = (double)b - d * (1.0 - t);
    return r;
}
// float32 images under NumPy 2: subtract(b, a) of the two float32 order statistics is a float32 difference (one
// rounding); gamma is float64, so the product and the sum are float64 operations on the widened values
__device__ __forceinline__ double pp_lerp(float a, float b, double t)
{
    const double d = (double)(b - a);
    double r = (double)a + d * t;
    if (t >= 0.5) r = (double)b - d * (1.0 - t);
    return r;
}

// ---- identity tiles of a float32 image (vmin == vmax: saturate_roi hands the float32 view on and denoise_roi stays in
// float32).  The working copy holds the float32 values widened to double; every stage rounds to float32 where NumPy /
// SciPy store one: np.clip against the float32 casts of the Python bounds, correlate1d's double accumulator stored
// into a float32 array after each axis pass (pp_round32), the unsharp mask's three float32 operations.
__device__ __forceinline__ double pp_round32(double v) { return (double)(float)v; }
__device__ __forceinline__ double pp_clip32(double x, double lo, double hi)
{
    return (double)fminf(fmaxf((float)x, (float)lo), (float)hi);
}
__device__ __forceinline__ double pp_unsharp32(double den, double blur, double strength)
{
    const float m = (float)strength * (float)blur;
    const float hp = (float)den - m;
    return (double)((float)den + hp);
}

// saturate_roi's stretch (clip(x, vmin, vmax) - vmin) / span.  The division is IEEE-exact: it is the
// compiler's own float64 expansion (v_div_scale / v_rcp + 2 Newton steps / q = n*r; e = fma(-d, q, n);
// v_div_fmas; v_div_fixup) with the denominator-only part hoisted out of the voxel loop.  That is valid
// while v_div_scale leaves both operands unscaled, i.e. for ordinary magnitudes: `fast` is set only
// when 2^-200 < span < 2^200, and the numerator is 0 or in [2^-60, span] (a difference of a <= 16-bit
// integer and an interpolated one).  Otherwise the plain `/` is used.
// An *identity* tile (vmin == vmax: the reference leaves the voxels alone) runs the same formula with
// vmin = 0, vmax = +inf, span = 1, which returns x exactly.
// SIGNED (int16 voxels): the identity form must not clip negative voxels at its stand-in vmin = 0, so the clip's lower
// bound is a member of its own (-inf on an identity tile, vmin otherwise); the unsigned form is as it always was.
template <bool SIGNED>
struct pp_sat_t {
    double vmin, vmax, span, rcp, clo;
    int identity, fast;
    // from the bounds of a tile (pp_key_bounds / pp_make_bounds, or the tile's info record)
    static __device__ __forceinline__ pp_sat_t make(double vmin, double vmax, int identity)
    {
        pp_sat_t S;
        S.identity = identity;
        S.vmin = vmin; S.vmax = vmax; S.span = vmax - vmin;
        S.finish();
        return S;
    }
    __device__ __forceinline__ double lower() const { return SIGNED ? clo : vmin; }
    __device__ __forceinline__ void finish()
    {
        clo = vmin;
        if (identity) { vmin = 0.; vmax = __builtin_inf(); span = 1.; clo = -__builtin_inf(); }
        fast = span > 0x1p-200 && span < 0x1p200;
        double r = __builtin_amdgcn_rcp(span);
        r = __builtin_fma(__builtin_fma(-span, r, 1.0), r, r);
        r = __builtin_fma(__builtin_fma(-span, r, 1.0), r, r);
        rcp = r;
    }
    __device__ __forceinline__ double operator()(double raw) const      // requires `fast`
    {
        const double num = pp_clip(raw, lower(), vmax) - vmin;
        const double q = num * rcp;
        const double e = __builtin_fma(-span, q, num);
        return __builtin_fma(e, rcp, q);
    }
    __device__ __forceinline__ double plain(double raw) const            // any magnitude
    {
        return (pp_clip(raw, lower(), vmax) - vmin) / span;
    }
};

// The voxel types of the integer kernels.  Histograms, the radix select and every "no voxel" sentinel work on the
// order-preserving KEY of the type, value + bias (mmx_key).  lerp: NumPy's _lerp on the two order statistics, whose
// difference NumPy takes IN THE VOXEL TYPE -- for int16 it wraps, and np.percentile returns what follows from the
// wrapped difference.
template <typename InT> struct pp_vox {
    static constexpr int bias = mmx_key<InT>::bias;
    static constexpr bool is_signed = false;
    static __device__ __forceinline__ double lerp(int ka, int kb, double t) { return pp_lerp(ka, kb, t); }
};
template <> struct pp_vox<int16_t> {
    static constexpr int bias = mmx_key<int16_t>::bias;
    static constexpr bool is_signed = true;
    static __device__ __forceinline__ double lerp(int ka, int kb, double t)
    {
        const int a = ka - bias, b = kb - bias;
        const double d = (double)(int16_t)(b - a);
        double r = (double)a + d * t;
        if (t >= 0.5) r = (double)b - d * (1.0 - t);
        return r;
    }
};

// histogram increment with the lanes that share the first active lane's bin folded into one LDS
// atomic: a tile is mostly background, whose voxels all land in one or two bins
__device__ __forceinline__ void pp_hist_add(uint32_t* hist, int bin, bool active)
{
    const unsigned long long act = __ballot(active);
    if (!act) return;
    const int leader = __ffsll((long long)act) - 1;
    const int lead_bin = __shfl(bin, leader);
    const unsigned long long same = __ballot(active && bin == lead_bin);
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[lead_bin], (uint32_t)__popcll(same));
    if (active && bin != lead_bin) atomicAdd(&hist[bin], 1u);
}

// Executed by one full wave: the bin of `h[0..255]` holding 0-based rank `rank`, and the rank
// inside that bin.
__device__ __forceinline__ void pp_select(const uint32_t* h, uint32_t rank, int& bin, uint32_t& res)
{
    const int lane = threadIdx.x & 63;
    const uint32_t c0 = h[4 * lane], c1 = h[4 * lane + 1], c2 = h[4 * lane + 2], c3 = h[4 * lane + 3];
    const uint32_t s = c0 + c1 + c2 + c3;
    uint32_t incl = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    const uint32_t excl = incl - s;
    const bool mine = rank >= excl && rank < incl;
    const unsigned long long m = __ballot(mine);
    const int src = m ? __ffsll((long long)m) - 1 : 63;
    uint32_t r = rank - excl;
    int b = 4 * lane;
    if (r >= c0) { r -= c0; ++b; if (r >= c1) { r -= c1; ++b; if (r >= c2) { r -= c2; ++b; } } }
    bin = __shfl(b, src);
    res = __shfl(r, src);
}

// ---- the four order statistics of a tile of 16-bit keys: a two-level radix select.  hist[0..255] is the kernel's own
// histogram of the high bytes; hist[256 (1 + s) ..] the low-byte histogram of the s-th DISTINCT high-byte bin the
// ranks fall in (prev / next ranks usually share theirs).  Barriers between the steps are the caller's.
struct pp_ranks { int bin[4]; uint32_t res[4]; int val[4]; };        // (LDS) high-byte bin, rank inside it, the key

// waves 0..3: the high-byte bin of rank lo_prev / lo_next / hi_prev / hi_next
// (qc by value: through a reference the class's loads sink into the guarded region and every kernel gains four
//  exec-mask regions; pp_stats_kernel, which takes one more VGPR from this helper, keeps the step pasted)
__device__ __forceinline__ void pp_select_high(const uint32_t* hist, mmx_quantile_class qc, pp_ranks* R)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave < 4) {
        const uint32_t rank = wave == 0 ? qc.lo_prev : wave == 1 ? qc.lo_next : wave == 2 ? qc.hi_prev : qc.hi_next;
        int b; uint32_t r;
        pp_select(hist, rank, b, r);
        if (lane == 0) { R->bin[wave] = b; R->res[wave] = r; }
    }
}

// the distinct bins among the four, in registers; add(): one voxel into the low-byte histogram of its bin
struct pp_bins {
    int b0, b1, b2, b3;
    bool u1, u2, u3;
    __device__ __forceinline__ explicit pp_bins(const pp_ranks* R)
        : b0(R->bin[0]), b1(R->bin[1]), b2(R->bin[2]), b3(R->bin[3]),
          u1(b1 != b0), u2(b2 != b0 && b2 != b1), u3(b3 != b0 && b3 != b1 && b3 != b2) {}
    __device__ __forceinline__ void add(uint32_t* hist, int key) const
    {
        const int hi = key >> 8, lo = key & 255;
        if (hi == b0) atomicAdd(&hist[256 + lo], 1u);
        if (u1 && hi == b1) atomicAdd(&hist[512 + lo], 1u);
        if (u2 && hi == b2) atomicAdd(&hist[768 + lo], 1u);
        if (u3 && hi == b3) atomicAdd(&hist[1024 + lo], 1u);
    }
};

// waves 0..3: the key of the wave's rank, from the low-byte histogram of the first slot that holds its bin
__device__ __forceinline__ void pp_select_low(const uint32_t* hist, pp_ranks* R)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave < 4) {
        int slot = wave;
        for (int w = wave - 1; w >= 0; --w) if (R->bin[w] == R->bin[wave]) slot = w;
        int b; uint32_t r;
        pp_select(hist + 256 * (1 + slot), R->res[wave], b, r);
        if (lane == 0) R->val[wave] = (R->bin[wave] << 8) | b;
    }
}

// ---- saturate_roi's bounds: the two percentiles, `identity` (vmin == vmax, tested BEFORE max_thresh raises vmax)
struct pp_bounds { double vmin, vmax; int identity; };
__device__ __forceinline__ pp_bounds pp_make_bounds(double vmin, double vmax, double max_thresh)
{
    pp_bounds B;
    B.identity = vmin == vmax;
    if (vmax < max_thresh) vmax = max_thresh;
    B.vmin = vmin; B.vmax = vmax;
    return B;
}
template <typename InT>
__device__ __forceinline__ pp_bounds pp_key_bounds(const pp_ranks* R, mmx_quantile_class qc, double max_thresh)
{
    return pp_make_bounds(pp_vox<InT>::lerp(R->val[0], R->val[1], qc.lo_gamma),
                          pp_vox<InT>::lerp(R->val[2], R->val[3], qc.hi_gamma), max_thresh);
}

// ---- np.mean(saturated) gates the erosion: the tile's flags from a mean summed in any order.  Where that mean lands
// within 1e-9 (relative to max(1, |threshold|)) of the threshold, NumPy's own summation order decides: at_knife(mean)
// either replaces the mean by the pairwise sum and returns pp_exact_verdict of it, or returns MMX_PP_KNIFE to leave
// both to a later kernel.
__device__ __forceinline__ int pp_exact_verdict(double mean, const pp_args& A)      // of a mean summed in NumPy's order
{
    return MMX_PP_EXACT_MEAN | (mean > A.ero_thr ? MMX_PP_ERODED : 0);
}
template <typename Knife>
__device__ __forceinline__ int pp_mean_verdict(double& mean, bool identity, const pp_args& A, Knife at_knife)
{
    int flags = identity ? MMX_PP_IDENTITY : 0;
    if (A.do_erosion) {
        const double tol = 1e-9 * (fabs(A.ero_thr) > 1. ? fabs(A.ero_thr) : 1.);
        if (!identity && fabs(mean - A.ero_thr) <= tol) flags |= at_knife(mean);
        else if (mean > A.ero_thr) flags |= MMX_PP_ERODED;
    }
    return flags;
}

__device__ __forceinline__ void pp_write_info(mmx_subblock_info* info, int id, double vmin, double vmax, double mean,
                                              int flags)
{
    mmx_subblock_info o;
    o.vmin = vmin; o.vmax = vmax; o.mean = mean; o.flags = flags; o._pad = 0;
    info[id] = o;
}

// ---- den + (den - strength * blur): three roundings, in this order (the kernels are built with -ffp-contract=off)
__device__ __forceinline__ double pp_unsharp(double den, double blur, double strength)
{
    const double m = strength * blur;
    const double hp = den - m;
    return den + hp;
}

// ---- grey_erosion with octahedron(1): the minimum over a voxel and the neighbours it has ('reflect' == skip outside).
// t[pos] is the voxel, py / pz the row and plane pitches (x pitch 1).
template <typename I>
__device__ __forceinline__ double pp_erode7(const double* t, I pos, I py, I pz, bool xm, bool xp, bool ym, bool yp,
                                            bool zm, bool zp)
{
    double o = t[pos];
    if (xm) o = fmin(o, t[pos - 1]);
    if (xp) o = fmin(o, t[pos + 1]);
    if (ym) o = fmin(o, t[pos - py]);
    if (yp) o = fmin(o, t[pos + py]);
    if (zm) o = fmin(o, t[pos - pz]);
    if (zp) o = fmin(o, t[pos + pz]);
    return o;
}

// both output copies of one voxel (the float32 copy feeds the LoG passes)
__device__ __forceinline__ void pp_put(double* __restrict__ out64, float* __restrict__ out32, int64_t d, double o)
{
    out64[d] = o;
    out32[d] = (float)o;
}

__device__ __forceinline__ double pp_wave_sum(double v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
    return v;
}

// NumPy's pairwise summation of val(0..n-1) (DOUBLE_pairwise_sum), by ONE lane.  `stk` is
// 4 x 40 ints/doubles of LDS for the explicit recursion stack.
template <typename F>
__device__ double pp_pairwise_leaf(F val, int lo, int n)
{
    if (n < 8) {
        double res = 0.;
        for (int i = 0; i < n; ++i) res += val(lo + i);
        return res;
    }
    double r0 = val(lo), r1 = val(lo + 1), r2 = val(lo + 2), r3 = val(lo + 3);
    double r4 = val(lo + 4), r5 = val(lo + 5), r6 = val(lo + 6), r7 = val(lo + 7);
    int i;
    for (i = 8; i < n - (n % 8); i += 8) {
        r0 += val(lo + i); r1 += val(lo + i + 1); r2 += val(lo + i + 2); r3 += val(lo + i + 3);
        r4 += val(lo + i + 4); r5 += val(lo + i + 5); r6 += val(lo + i + 6); r7 += val(lo + i + 7);
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += val(lo + i);
    return res;
}

struct pp_stack { int lo[40]; int n[40]; int st[40]; double acc[40]; };

template <typename F>
__device__ double pp_pairwise(F val, int n, pp_stack* S)
{
    int sp = 0;
    double ret = 0.;
    S->lo[0] = 0; S->n[0] = n; S->st[0] = 0; sp = 1;
    while (sp > 0) {
        const int t = sp - 1;
        const int lo = S->lo[t], m = S->n[t];
        if (m <= 128) { ret = pp_pairwise_leaf(val, lo, m); --sp; continue; }
        int n2 = m / 2; n2 -= n2 % 8;
        if (S->st[t] == 0) { S->st[t] = 1; S->lo[sp] = lo; S->n[sp] = n2; S->st[sp] = 0; ++sp; }
        else if (S->st[t] == 1) {
            S->acc[t] = ret; S->st[t] = 2;
            S->lo[sp] = lo + n2; S->n[sp] = m - n2; S->st[sp] = 0; ++sp;
        } else { ret = S->acc[t] + ret; --sp; }
    }
    return 0. + ret;   // the reduction starts from the identity (add.reduce)
}

// NumPy's pairwise summation tree evaluated in parallel: the leaves (runs of <= 128 elements, fixed by n alone)
// are enumerated once per tile, every lane sums whole leaves (pp_pairwise_leaf, NumPy's 8 accumulators), one
// lane folds the leaf sums in the tree's order.  Bit-equal to ndarray.sum() of a contiguous float64 array.
struct pp_leaves { int lo[PP_MAXLEAF]; int n[PP_MAXLEAF]; double sum[2][PP_MAXLEAF]; int count; };

__device__ void pp_enum_leaves(int n, pp_stack* S, pp_leaves* Lv)       // one lane
{
    int sp = 0, cnt = 0;
    S->lo[0] = 0; S->n[0] = n; sp = 1;
    while (sp > 0) {
        --sp;
        const int lo = S->lo[sp], m = S->n[sp];
        if (m <= 128) {
            if (cnt < PP_MAXLEAF) { Lv->lo[cnt] = lo; Lv->n[cnt] = m; }
            ++cnt;
            continue;
        }
        int n2 = m / 2; n2 -= n2 % 8;
        S->lo[sp] = lo + n2; S->n[sp] = m - n2; ++sp;       // right half: popped after the left one
        S->lo[sp] = lo; S->n[sp] = n2; ++sp;
    }
    Lv->count = cnt;
}

__device__ double pp_fold_leaves(int n, pp_stack* S, const pp_leaves* Lv, int which)     // one lane
{
    int sp = 0, next = 0;
    double ret = 0.;
    S->lo[0] = 0; S->n[0] = n; S->st[0] = 0; sp = 1;
    while (sp > 0) {
        const int t = sp - 1;
        const int lo = S->lo[t], m = S->n[t];
        if (m <= 128) { ret = Lv->sum[which][next++]; --sp; continue; }
        int n2 = m / 2; n2 -= n2 % 8;
        if (S->st[t] == 0) { S->st[t] = 1; S->lo[sp] = lo; S->n[sp] = n2; S->st[sp] = 0; ++sp; }
        else if (S->st[t] == 1) {
            S->acc[t] = ret; S->st[t] = 2;
            S->lo[sp] = lo + n2; S->n[sp] = m - n2; S->st[sp] = 0; ++sp;
        } else { ret = S->acc[t] + ret; --sp; }
    }
    return 0. + ret;
}

// One in-place Gaussian pass over the lines of one axis, lines held in registers.
// base/stride address the LDS tile; L <= PP_MAXL.
// The weights come through a `const __restrict__` kernel argument (scalar loads next to their use),
// not by value: 66 SGPRs held from kernel entry made the compiler spill scalars in every other stage.
template <int MAXL = PP_MAXL>
__device__ __forceinline__ void pp_line_pass(double* __restrict__ tile, int64_t base, int64_t stride, int L,
                                             const double (&w)[PP_R + 1])
{
    double r[MAXL];
#pragma unroll
    for (int i = 0; i < MAXL; ++i) r[i] = tile[base + (i < L ? i : L - 1) * stride];
#pragma unroll
    for (int i = 0; i < MAXL; ++i) {
        if (i < L) {
            double acc = r[i] * w[0];
#pragma unroll
            for (int k = PP_R; k >= 1; --k) {
                const int a = i - k < 0 ? 0 : i - k;
                const int b = i + k > MAXL - 1 ? MAXL - 1 : i + k;
                acc += (r[a] + r[b]) * w[k];
            }
            tile[base + i * stride] = acc;
        }
    }
}

inline pp_args pp_make_args(const mmx_preproc_params* p, int64_t dst_sy, int64_t dst_sz)
{
    pp_args A;
    A.clip_min = p->clip_min; A.clip_max = p->clip_max; A.max_thresh = p->max_thresh;
    A.strength = p->unsharp_strength; A.ero_thr = p->erosion_threshold;
    A.tv_weight = p->tv_weight; A.tv_factor = p->tv_factor;
    A.dst_sy = dst_sy; A.dst_sz = dst_sz;
    A.do_unsharp = p->unsharp_strength != 0.0;          // Python truthiness: `if unsharp_strength:`
    A.do_erosion = p->erosion_threshold != 0.0;         // `if thresh_eros and ...`
    A.rgb_guess = p->rgb_guess;
    A._pad = 0;
    return A;
}

}  // namespace

// mmx_preproc_pipe.hip
int64_t mmx_pp_pipe_work_bytes(const mmx_subblock* h_subs, int n_subs);
int mmx_launch_pp_pipe(const mmx_volume* vol, const mmx_subblock* d_subs, const mmx_subblock* h_subs, int n_subs,
                       const mmx_quantile_class* d_qclasses, const double* d_weights, const pp_args& A,
                       float* d_out32, double* d_out64, mmx_subblock_info* d_info, void* d_work,
                       int tiles_per_wg, hipStream_t s);
