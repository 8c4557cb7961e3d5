// The leading eigenpairs of a resident symmetric matrix by blocked subspace iteration with Rayleigh-Ritz.  The contract is in
// include/malva_hip.h (mg_pca_solve), the geometry in pca_plan.h, the method's restatement in tests/pca_model.py.  The reference -- one
// individual per run -- has nothing like it.
//
// Resident state: G [np][np] doubles, np = n rounded up to 16, symmetric by construction and 0 in rows and columns n .. np - 1; the blocks
// (Q, Y and two spares) [np][m] row-major, 0 in rows n .. np - 1.  The pad is KEPT ZERO, not guarded: the load writes it, pca_fill_kernel
// writes it, and every other kernel maps zero rows to zero rows, so a pad row adds +0.0 to a sum and nothing else.
//
// Load (pca_expand_kernel<T>): a thread per element of the padded matrix.  (i, j) reads the lower-triangle element (max, min) of a packed
// float triangle or of a full double array, so the upper triangle of a full array is never read.  A non-finite value raises an integer
// flag (an atomic OR: no order to depend on).
//
// Product (pca_product_kernel<CT>): Y = G Q on v_mfma_f64_16x16x4_f64, CT = m / 16 accumulator tiles per wave (4 doubles a lane each).
// The A fragment of lane l is G[row0 + (l & 15)][k + (l >> 4)]; it is loaded as G[k + (l >> 4)][row0 + (l & 15)] -- the same value, G being
// symmetric -- so that a wave's load is four 128-byte runs instead of sixteen 32-byte ones.  B: Q[k + (l >> 4)][16 c + (l & 15)].  C/D of
// the f64 form: column = lane & 15, row = (lane >> 4) + 4 register.  A workgroup's four waves take a quarter of its k chunk each and add
// their tiles through LDS in wave order; with more than one split the workgroups write partial blocks that pca_sum_parts_kernel adds in
// split order.  Nothing is atomic, so the order of every sum is fixed by n.
//
// Reductions (pca_gram_part_kernel, pca_gram_sum_kernel): C = A^T B, m x m, from two [np][m] blocks.  First stage: a workgroup per
// PCA_RED_ROWS rows, 256 threads, thread (ti, tj) owns the entries (ti + 16 a, tj + 16 b) and adds its rows in order from LDS.  Second
// stage: a thread per entry adds the workgroups' tables in order.
//
// Orthonormalisation: Cholesky QR twice.  W = Y^T Y by the reduction; pca_chol_kernel (one workgroup) factors W = R^T R in LDS, inverts R, and
// marks a column as collapsed when its pivot is not above PCA_COLLAPSE of the column's own squared norm (or the norm is nothing beside
// the largest): such a column leaves the factor (its row and column of R are dropped, its column of R^-1 is 0).  Q = Y R^-1 by the block
// update; pca_fill_kernel then writes fresh hashed vectors into the marked columns, and the second pass orthonormalises them against the
// rest.  The block keeps its full width whatever the rank of G.
//
// Block update (pca_update_kernel): Out = In S, [np][m] times [m][m], S in LDS.  Residual norms (pca_resid_kernel): a workgroup per
// column, thread t adds rows t, t + 256, .. in order, then a fixed LDS tree.  Sign rule and output (pca_emit_kernel): a workgroup per
// returned component finds the component of largest magnitude (lowest index among equals) by the same tree and writes the row, negated
// when that component is negative.
#pragma once
#include "pca_plan.h"

namespace {
using namespace mg;

constexpr u32 PCA_TPB = 256;
constexpr double PCA_COLLAPSE = 1e-10, PCA_NOTHING = 1e-60;

template <typename T> struct PcaExpandArgs {
    const T *src;
    double *g;
    u32 n, np;
    int packed; // the lower triangle row by row, else [n][n] row-major
    u32 *bad;
};

// grid: ceil(np np / PCA_TPB)
template <typename T> __global__ void __launch_bounds__(PCA_TPB) pca_expand_kernel(PcaExpandArgs<T> a)
{
    const u64 at = (u64)blockIdx.x * PCA_TPB + threadIdx.x;
    if (at >= (u64)a.np * a.np) return;
    const u32 i = (u32)(at / a.np), j = (u32)(at % a.np);
    double x = 0.0;
    if (i < a.n && j < a.n) {
        const u64 hi = i > j ? i : j, lo = i > j ? j : i;
        x = (double)a.src[a.packed ? hi * (hi + 1) / 2 + lo : hi * a.n + lo];
        if (!(fabs(x) <= 1.79769313486231570815e308)) atomicOr(a.bad, 1u);
    }
    a.g[at] = x;
}

// a block's columns `only` (all of them when only == nullptr) from the counter hash; rows n .. np - 1 are 0.  grid: ceil(np m / PCA_TPB)
__global__ void __launch_bounds__(PCA_TPB) pca_fill_kernel(double *q, u32 n, u32 np, u32 m, u64 salt, const u32 *only)
{
    const u64 at = (u64)blockIdx.x * PCA_TPB + threadIdx.x;
    if (at >= (u64)np * m) return;
    const u32 i = (u32)(at / m), j = (u32)(at % m);
    if (only && !only[j]) return;
    q[at] = i < n ? pca_hash_value(i, j, salt) : 0.0;
}

typedef double pca_v4d __attribute__((ext_vector_type(4)));

struct PcaProductArgs {
    const double *g, *q;
    double *out; // [splits][np][m]
    u32 np, m, chunk;
};

// grid: (np / 16, splits); 4 waves
template <int CT> __global__ void __launch_bounds__(64 * PCA_WAVES) pca_product_kernel(PcaProductArgs a)
{
    __shared__ double part[PCA_WAVES][CT][4][64];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, kq = lane >> 4;
    const u32 row0 = blockIdx.x * PCA_TILE, quarter = a.chunk / PCA_WAVES;
    const u32 k_begin = blockIdx.y * a.chunk + wave * quarter, k_stop = k_begin + quarter < a.np ? k_begin + quarter : a.np;
    pca_v4d acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[c] = pca_v4d{0.0, 0.0, 0.0, 0.0};
    const double *gp = a.g + (u64)(k_begin + kq) * a.np + row0 + r, *qp = a.q + (u64)(k_begin + kq) * a.m + r;
    u32 k = k_begin; // (k_begin, k_stop and np are multiples of 4: rows k + kq < np)
    for (; k + 4 * PCA_MFMA_K <= k_stop; k += 4 * PCA_MFMA_K) { // four steps' loads in flight, the products in k order
        double ga[4], qb[4][CT];
#pragma unroll
        for (u32 u = 0; u < 4; ++u) {
            ga[u] = gp[(u64)u * PCA_MFMA_K * a.np];
#pragma unroll
            for (int c = 0; c < CT; ++c) qb[u][c] = qp[(u64)u * PCA_MFMA_K * a.m + 16 * c];
        }
#pragma unroll
        for (u32 u = 0; u < 4; ++u)
#pragma unroll
            for (int c = 0; c < CT; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(ga[u], qb[u][c], acc[c], 0, 0, 0);
        gp += (u64)4 * PCA_MFMA_K * a.np;
        qp += (u64)4 * PCA_MFMA_K * a.m;
    }
    for (; k < k_stop; k += PCA_MFMA_K) {
        const double ga = *gp;
        double qb[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) qb[c] = qp[16 * c];
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(ga, qb[c], acc[c], 0, 0, 0);
        gp += (u64)PCA_MFMA_K * a.np;
        qp += (u64)PCA_MFMA_K * a.m;
    }
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) part[wave][c][e][lane] = acc[c][e];
    __syncthreads();
    double *out = a.out + (u64)blockIdx.y * a.np * a.m;
    for (u32 t = threadIdx.x; t < CT * 4 * 64; t += 64 * PCA_WAVES) {
        const u32 l = t & 63, e = (t >> 6) & 3, c = t >> 8;
        double s = part[0][c][e][l];
#pragma unroll
        for (u32 w = 1; w < PCA_WAVES; ++w) s += part[w][c][e][l];
        out[(u64)(row0 + (l >> 4) + 4 * e) * a.m + 16 * c + (l & 15)] = s;
    }
}

// y = part[0] + part[1] + .. in order.  grid: ceil(np m / PCA_TPB)
__global__ void __launch_bounds__(PCA_TPB) pca_sum_parts_kernel(const double *part, u32 splits, u64 count, double *y)
{
    const u64 at = (u64)blockIdx.x * PCA_TPB + threadIdx.x;
    if (at >= count) return;
    double s = part[at];
    for (u32 p = 1; p < splits; ++p) s += part[p * count + at];
    y[at] = s;
}

// part[block] = A[rows of the block]^T B[the same rows], [m][m].  grid: pca_red_blocks(np); 256 threads
__global__ void __launch_bounds__(PCA_TPB) pca_gram_part_kernel(const double *a, const double *b, u32 np, u32 m, double *part)
{
    constexpr u32 ROWS = 16;
    __shared__ double sa[ROWS][PCA_MAX_BLOCK], sb[ROWS][PCA_MAX_BLOCK];
    const u32 ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
    const u32 row_begin = blockIdx.x * PCA_RED_ROWS, row_stop = row_begin + PCA_RED_ROWS < np ? row_begin + PCA_RED_ROWS : np;
    double acc[4][4];
#pragma unroll
    for (u32 x = 0; x < 4; ++x)
#pragma unroll
        for (u32 y = 0; y < 4; ++y) acc[x][y] = 0.0;
    for (u32 r0 = row_begin; r0 < row_stop; r0 += ROWS) { // (np is a multiple of 16: whole slabs)
        for (u32 t = threadIdx.x; t < ROWS * m; t += PCA_TPB) {
            const u32 rr = t / m, cc = t % m;
            sa[rr][cc] = a[(u64)(r0 + rr) * m + cc];
            sb[rr][cc] = b[(u64)(r0 + rr) * m + cc];
        }
        __syncthreads();
        for (u32 rr = 0; rr < ROWS; ++rr)
#pragma unroll
            for (u32 x = 0; x < 4; ++x)
#pragma unroll
                for (u32 y = 0; y < 4; ++y)
                    if (ti + 16 * x < m && tj + 16 * y < m) acc[x][y] += sa[rr][ti + 16 * x] * sb[rr][tj + 16 * y];
        __syncthreads();
    }
#pragma unroll
    for (u32 x = 0; x < 4; ++x)
#pragma unroll
        for (u32 y = 0; y < 4; ++y)
            if (ti + 16 * x < m && tj + 16 * y < m) part[(u64)blockIdx.x * m * m + (u64)(ti + 16 * x) * m + tj + 16 * y] = acc[x][y];
}

// c = part[0] + part[1] + .. in order.  grid: ceil(m m / PCA_TPB)
__global__ void __launch_bounds__(PCA_TPB) pca_gram_sum_kernel(const double *part, u32 blocks, u32 mm, double *c)
{
    const u32 at = blockIdx.x * PCA_TPB + threadIdx.x;
    if (at >= mm) return;
    double s = part[at];
    for (u32 p = 1; p < blocks; ++p) s += part[(u64)p * mm + at];
    c[at] = s;
}

// W [m][m] (its upper triangle is read) -> rinv [m][m], the inverse of the Cholesky factor R (W = R^T R) over the columns that did not
// collapse, 0 in the row and column of one that did; flags[j] = 1 for a collapsed column j, else 0.  One workgroup of 256 threads: the
// trailing block of a step is spread over all of them, every entry losing its products in step order; then thread t solves R x = e_t for
// column t of the inverse, keeping x below the diagonal of the factor's own table (row t, conflict-free through the padded row).
__global__ void __launch_bounds__(PCA_TPB) pca_chol_kernel(const double *w, u32 m, double *rinv, u32 *flags)
{
    __shared__ double s[PCA_MAX_BLOCK][PCA_MAX_BLOCK + 1];
    __shared__ double diag0[PCA_MAX_BLOCK];
    __shared__ u32 dead[PCA_MAX_BLOCK];
    const u32 t = threadIdx.x;
    for (u32 e = t; e < m * m; e += PCA_TPB) {
        const u32 i = e / m, c = e % m;
        s[i][c] = i <= c ? w[e] : 0.0;
    }
    if (t < m) diag0[t] = w[(u64)t * m + t];
    __syncthreads();
    double wmax = 0.0;
    for (u32 j = 0; j < m; ++j) wmax = diag0[j] > wmax ? diag0[j] : wmax;
    // right-looking: after step j, row j holds R's row j and the trailing block has lost its outer product
    for (u32 j = 0; j < m; ++j) {
        const double d = s[j][j];
        const bool gone = !(d > PCA_COLLAPSE * diag0[j] && diag0[j] > PCA_NOTHING * wmax); // (the same in every thread)
        __syncthreads();
        if (t == j) dead[j] = gone;
        if (t >= j && t < m) s[j][t] = gone ? 0.0 : s[j][t] / sqrt(d);
        __syncthreads();
        if (!gone) {
            const u32 side = m - j - 1;
            for (u32 e = t; e < side * side; e += PCA_TPB) {
                const u32 i = j + 1 + e / side, c = j + 1 + e % side;
                if (i <= c) s[i][c] -= s[j][i] * s[j][c];
            }
        }
        __syncthreads();
    }
    // column t of R^-1 by back substitution over the live rows: x[i], i < t, lives at s[t][i] (0 so far), x[t] in a register
    if (t < m) {
        double xt = 0.0;
        if (!dead[t]) {
            xt = 1.0 / s[t][t];
            for (u32 ii = t; ii-- > 0;) {
                if (dead[ii]) continue;
                double acc = 0.0;
                for (u32 k = ii + 1; k < t; ++k) acc += s[ii][k] * s[t][k];
                acc += s[ii][t] * xt;
                s[t][ii] = -acc / s[ii][ii];
            }
        }
        for (u32 i = 0; i < m; ++i) rinv[(u64)i * m + t] = i < t ? s[t][i] : i == t ? xt : 0.0;
        flags[t] = dead[t];
    }
}

// out = in S.  grid: ceil(np / 64); thread (row, quarter of the columns)
__global__ void __launch_bounds__(PCA_TPB) pca_update_kernel(const double *in, const double *sm, u32 np, u32 m, double *out)
{
    __shared__ double s[PCA_MAX_BLOCK][PCA_MAX_BLOCK];
    for (u32 t = threadIdx.x; t < m * m; t += PCA_TPB) s[t / m][t % m] = sm[t];
    __syncthreads();
    const u32 row = blockIdx.x * 64 + (threadIdx.x >> 2), c0 = (threadIdx.x & 3) * (m / 4), nc = m / 4; // (m is a multiple of 16)
    if (row >= np) return;
    double acc[PCA_MAX_BLOCK / 4];
#pragma unroll
    for (u32 c = 0; c < PCA_MAX_BLOCK / 4; ++c) acc[c] = 0.0;
    const double *x = in + (u64)row * m;
    for (u32 k = 0; k < m; ++k) {
        const double xk = x[k];
#pragma unroll
        for (u32 c = 0; c < PCA_MAX_BLOCK / 4; ++c)
            if (c < nc) acc[c] += xk * s[k][c0 + c];
    }
#pragma unroll
    for (u32 c = 0; c < PCA_MAX_BLOCK / 4; ++c)
        if (c < nc) out[(u64)row * m + c0 + c] = acc[c];
}

// norm[j] = || Y[:, j] - theta[j] Q[:, j] ||_2.  grid: m; 256 threads
__global__ void __launch_bounds__(PCA_TPB) pca_resid_kernel(const double *q, const double *y, const double *theta, u32 np, u32 m, double *norm)
{
    __shared__ double s[PCA_TPB];
    const u32 j = blockIdx.x;
    const double th = theta[j];
    double acc = 0.0;
    for (u32 i = threadIdx.x; i < np; i += PCA_TPB) {
        const double d = y[(u64)i * m + j] - th * q[(u64)i * m + j];
        acc += d * d;
    }
    s[threadIdx.x] = acc;
    __syncthreads();
    for (u32 w = PCA_TPB / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) norm[j] = sqrt(s[0]);
}

// vectors_out[j][0 .. n) = +- Q[0 .. n)[j], the component of largest magnitude positive (the lowest index among equals).  grid: k
__global__ void __launch_bounds__(PCA_TPB) pca_emit_kernel(const double *q, u32 n, u32 m, double *vectors_out)
{
    __shared__ double sv[PCA_TPB];
    __shared__ u32 si[PCA_TPB];
    const u32 j = blockIdx.x;
    double best = -1.0;
    u32 where = 0xFFFFFFFFu;
    for (u32 i = threadIdx.x; i < n; i += PCA_TPB) { // (ascending i: a later equal does not replace an earlier one)
        const double v = fabs(q[(u64)i * m + j]);
        if (v > best) best = v, where = i;
    }
    sv[threadIdx.x] = best;
    si[threadIdx.x] = where;
    __syncthreads();
    for (u32 w = PCA_TPB / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            const double v = sv[threadIdx.x + w];
            const u32 at = si[threadIdx.x + w];
            if (v > sv[threadIdx.x] || (v == sv[threadIdx.x] && at < si[threadIdx.x])) sv[threadIdx.x] = v, si[threadIdx.x] = at;
        }
        __syncthreads();
    }
    const bool flip = q[(u64)si[0] * m + j] < 0.0;
    for (u32 i = threadIdx.x; i < n; i += PCA_TPB) {
        const double v = q[(u64)i * m + j];
        vectors_out[(u64)j * n + i] = flip ? -v : v;
    }
}

} // namespace
