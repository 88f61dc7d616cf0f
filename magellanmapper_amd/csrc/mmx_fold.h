// The folded operator of MMX_ZX_THIN.  SciPy's "reflect" (d c b a | a b c d | d c b a) maps every tap of a symmetric
// kernel of radius R onto one of the n voxels of the axis; on an axis shorter than the kernel the 2 R + 1 taps of an
// output therefore read only n distinct values, and the pass is the dense n x n matrix
//   M[i][j] = sum of w[|p - i|] over the images p of j, p in {2 n m + j, 2 n m - 1 - j : m integer}, |p - i| <= R
// (for n = 1 every integer is an image of voxel 0 and M is the sum of all taps).  ONE function states it, for the
// kernels (mmx_thin.hip builds the matrices of its block in LDS with it) and for the host (mmx_fold_matrix: tests,
// tools/route_check.cpp): float weights in, a sum in double in ascending p -- additions only, nothing a compiler may
// contract, so host and device give the same bits --, rounded once to float.
#pragma once

#if defined(__HIPCC__)
#define MMX_FOLD_FN __host__ __device__ inline
#else
#define MMX_FOLD_FN inline
#endif

// floor(a / b) for b > 0
MMX_FOLD_FN int mmx_fold_floordiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// M[i][j] for weights w[0 .. radius], 0 <= i, j < n
MMX_FOLD_FN float mmx_fold_entry(const float* w, int radius, int n, int i, int j)
{
    const int period = 2 * n;
    // images 2 n m + j and 2 n m - 1 - j within [i - radius, i + radius]: the periods m that can hold one
    const int m_lo = mmx_fold_floordiv(i - radius - j, period), m_hi = mmx_fold_floordiv(i + radius + 1 + j, period);
    double acc = 0.0;
    for (int m = m_lo; m <= m_hi; ++m) {
        const int mirrored = period * m - 1 - j, direct = period * m + j;       // (mirrored < direct: ascending p)
        int d = mirrored - i;
        if (d < 0) d = -d;
        if (d <= radius) acc += (double)w[d];
        d = direct - i;
        if (d < 0) d = -d;
        if (d <= radius) acc += (double)w[d];
    }
    return (float)acc;
}

// the whole matrix, row-major (out[i * n + j]), on the host
inline void mmx_fold_matrix_host(const float* w, int radius, int n, float* out)
{
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) out[i * n + j] = mmx_fold_entry(w, radius, n, i, j);
}
