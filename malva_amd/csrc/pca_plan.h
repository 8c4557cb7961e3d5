// pca_plan.h -- the geometry of mg_pca_solve (pca_kernels.h) and its small dense eigenproblem.  Plain C++, no HIP: the library includes it
// (malva_hip.hip first, then pca_kernels.h for the constants) and tools/pca_host_check.cpp compiles it by itself.
//
// Everything here is a function of n (and k) alone, never of the device or of what else runs on it: the split of an n-long dot product
// over waves and workgroups is part of the result's definition, because it fixes the order of the floating-point sums.
//   resident matrix   np x np doubles, np = n rounded up to PCA_TILE; rows and columns n .. np - 1 are written as 0 by the load and stay 0
//   block             m = min(n, roundup16(max(2 k, k + 16))) columns; the blocks Q, Y are [np][m] row-major, rows n .. np - 1 zero
//   product           one workgroup of PCA_WAVES waves per 16-row tile of Y and per split; the split's np-long k range is cut into `splits`
//                     workgroup chunks (a multiple of 4 PCA_WAVES), each wave of a workgroup taking a quarter in k order; the waves'
//                     partial tiles are added in wave order, the workgroups' in split order
//   reductions        Q^T Y and Y^T Y: PCA_RED_ROWS rows per first-stage workgroup, row order inside; the second stage adds the partial
//                     m x m tables in workgroup order
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace mg {

constexpr uint32_t PCA_TILE = 16;      // v_mfma_f64_16x16x4_f64: rows of a tile, columns of a tile
constexpr uint32_t PCA_MFMA_K = 4;     // ... and its k
constexpr uint32_t PCA_WAVES = 4;      // waves of a product workgroup
constexpr uint32_t PCA_FILL = 1024;    // workgroups a product launch should have (256 CUs x 4); a small matrix is split along k
constexpr uint32_t PCA_MIN_CHUNK = 256; // ... into workgroup chunks no shorter than this
constexpr uint32_t PCA_MAX_SPLITS = 16;
constexpr uint32_t PCA_RED_ROWS = 256; // rows per first-stage workgroup of a tall-skinny reduction
constexpr uint32_t PCA_MAX_BLOCK = 64; // m at most (k <= 32)
constexpr uint32_t PCA_CHECK_EVERY = 4; // products between two Rayleigh-Ritz steps

inline uint32_t pca_np(uint32_t n) { return (n + PCA_TILE - 1) / PCA_TILE * PCA_TILE; }

inline uint32_t pca_block(uint32_t n, uint32_t k)
{
    const uint32_t want = 2 * k > k + 16 ? 2 * k : k + 16, m = (want + 15) / 16 * 16;
    return n < m ? n : m;
}

// -> the workgroups along k of a product; *chunk = the k range of one of them, a multiple of PCA_MFMA_K PCA_WAVES
inline uint32_t pca_splits(uint32_t np, uint32_t *chunk)
{
    const uint32_t tiles = np / PCA_TILE;
    uint32_t splits = 1;
    while (splits < PCA_MAX_SPLITS && tiles * splits < PCA_FILL && np / (2 * splits) >= PCA_MIN_CHUNK) splits *= 2;
    const uint32_t unit = PCA_MFMA_K * PCA_WAVES;
    *chunk = ((np + splits - 1) / splits + unit - 1) / unit * unit;
    return splits;
}

inline uint32_t pca_red_blocks(uint32_t np) { return (np + PCA_RED_ROWS - 1) / PCA_RED_ROWS; }

// The start vectors and the replacements of collapsed directions: a counter hash of (row, column, salt) -- the finaliser of splitmix64 over
// an odd-multiplier mix of the three -- mapped to (-1, 1).  tests/pca_model.py restates it.
constexpr double pca_hash_value(uint64_t row, uint64_t col, uint64_t salt)
{
    uint64_t x = row * 0x9E3779B97F4A7C15ull + col * 0xBF58476D1CE4E5B9ull + salt * 0x94D049BB133111EBull + 0x2545F4914F6CDD1Dull;
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (double)(x >> 11) * (1.0 / 4503599627370496.0) - 1.0; // 2^-52: [0, 2) - 1
}

// The small dense symmetric eigenproblem, n <= PCA_MAX_BLOCK, on the host in double: cyclic Jacobi (Rutishauser's form: a rotation per
// off-diagonal entry and sweep, entries that no longer change the diagonal set to 0, at most 64 sweeps).  a is [n][n] row-major; its
// upper triangle is read and destroyed.  w[n]: the eigenvalues, algebraically descending (equal values keep the order Jacobi left them
// in); v is [n][n] row-major, column j the unit eigenvector of w[j].  -> the sweeps it took, or -1 when 64 were not enough
inline int pca_jacobi(uint32_t n, double *a, double *w, double *v)
{
    std::vector<double> b(n), d(n), z(n, 0.0), u((size_t)n * n, 0.0);
    for (uint32_t i = 0; i < n; ++i) {
        u[(size_t)i * n + i] = 1.0;
        b[i] = d[i] = a[(size_t)i * n + i];
    }
    int sweeps = -1;
    for (int sweep = 1; sweep <= 64; ++sweep) {
        double sm = 0.0;
        for (uint32_t p = 0; p + 1 < n; ++p)
            for (uint32_t q = p + 1; q < n; ++q) sm += std::fabs(a[(size_t)p * n + q]);
        if (sm == 0.0) {
            sweeps = sweep - 1;
            break;
        }
        const double tresh = sweep < 4 ? 0.2 * sm / ((double)n * n) : 0.0;
        for (uint32_t p = 0; p + 1 < n; ++p)
            for (uint32_t q = p + 1; q < n; ++q) {
                double &apq = a[(size_t)p * n + q];
                const double g = 100.0 * std::fabs(apq);
                if (sweep > 4 && std::fabs(d[p]) + g == std::fabs(d[p]) && std::fabs(d[q]) + g == std::fabs(d[q])) {
                    apq = 0.0;
                    continue;
                }
                if (!(std::fabs(apq) > tresh)) continue;
                double h = d[q] - d[p], t;
                if (std::fabs(h) + g == std::fabs(h)) t = apq / h;
                else {
                    const double theta = 0.5 * h / apq;
                    t = 1.0 / (std::fabs(theta) + std::sqrt(1.0 + theta * theta));
                    if (theta < 0.0) t = -t;
                }
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c);
                h = t * apq;
                z[p] -= h, z[q] += h, d[p] -= h, d[q] += h;
                apq = 0.0;
                auto rot = [&](double &x, double &y) {
                    const double gx = x, hy = y;
                    x = gx - s * (hy + gx * tau);
                    y = hy + s * (gx - hy * tau);
                };
                for (uint32_t j = 0; j < p; ++j) rot(a[(size_t)j * n + p], a[(size_t)j * n + q]);
                for (uint32_t j = p + 1; j < q; ++j) rot(a[(size_t)p * n + j], a[(size_t)j * n + q]);
                for (uint32_t j = q + 1; j < n; ++j) rot(a[(size_t)p * n + j], a[(size_t)q * n + j]);
                for (uint32_t j = 0; j < n; ++j) rot(u[(size_t)j * n + p], u[(size_t)j * n + q]);
            }
        for (uint32_t i = 0; i < n; ++i) {
            b[i] += z[i];
            d[i] = b[i];
            z[i] = 0.0;
        }
    }
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    for (uint32_t i = 1; i < n; ++i) // (a stable insertion sort: n <= 64)
        for (uint32_t j = i; j > 0 && d[order[j]] > d[order[j - 1]]; --j) {
            const uint32_t t = order[j];
            order[j] = order[j - 1];
            order[j - 1] = t;
        }
    for (uint32_t j = 0; j < n; ++j) {
        w[j] = d[order[j]];
        for (uint32_t i = 0; i < n; ++i) v[(size_t)i * n + j] = u[(size_t)i * n + order[j]];
    }
    return sweeps;
}

} // namespace mg
