// Label generator of the NU problem on the device: the search of noma_uav_gen, datasets/noma_uav_gen.py,
// float64 like the reference.
//
// Per sample (3 users q = x0 y0 x1 y1 x2 y2): every point p = y * 401 + x of the integer grid [0, 400]^2 that lies in the
// users' triangle (edges and corners included), times every row s of the power table fs [nfs][3] (feasible_solution, smallest
// power first, built by the host with numpy's aranges).  Per point, once:
//   h[u] = sqrt(rou_0 / ((H^2 + dx_u^2) + dy_u^2)); ranks by h descending, equal h -> lower user index first (numpy's stable
//   argsort of -h); the rank-r user gets column r of the table;
//   S_r = the 3r entries of table ROWS u_0 .. u_{r-1} (the stronger users' INDICES used as row numbers; columns in the
//   users' rank order), added one after another -- the reference's np.sum(F[sorted_indices[:r]]).  It is one scalar per
//   point, unlike the evaluator rate_calc (dsg_nu_rate), which adds the stronger users' powers;
//   D_r = S_r + sigma^2 / h_r^2.
// Per row s: rate = (log2(1 + sinr_u0) + log2(1 + sinr_u1)) + log2(1 + sinr_u2) in USER order, with sinr of the rank-0 user
// (p0 * h0^2) / sigma^2 and of the rank-r user p_r / D_r.  The label is the first maximum over rows, then over points in grid
// order: the lexicographic best of (rate descending, p ascending, s ascending).
//
// Contraction is off and every expression keeps the reference's order; sqrt and division are IEEE, so h, S_r, D_r and the
// sinr match numpy's bit for bit.  Only log2 is a different (equally ~1 ulp) implementation than numpy's.
//
// Work split: pass 1 (k_nu_tiles) gives every sample `tiles` workgroups, each a run of `tile_pts` points of the sample's scan
// region; the workgroup lists the inside points of its run in LDS, one thread per listed point walks the whole table (the
// table address is wave-uniform: scalar loads through the constant cache, no LDS copy, so any nfs up to the cap streams the
// same way) and the workgroup reduces to its best (rate, p << 32 | s).  Pass 2 (k_nu_pick) reduces a sample's tiles in the
// same total order -- no float atomics, the result does not depend on scheduling -- and writes x, y, powers, rate.
// Scan region: the triangle's bounding box when the corners are integers (the inside test is then exact, so nothing outside
// the box can pass it) and the triangle is not degenerate; otherwise the whole grid, since the reference's test counts every
// point on the line of a degenerate (collinear) triangle as inside.
#pragma once
#include <hip/hip_runtime.h>

namespace dsg {

constexpr int kNuGrid = 401;                       // np.arange(0, 400 + 1)
constexpr int kNuGridPts = kNuGrid * kNuGrid;
constexpr int kNuMaxSolutions = 16384;             // P_sum = 30 has 9 696 rows
constexpr int kNuThreads = 256;
constexpr int kNuMaxTile = 4096;                   // points per pass-1 workgroup, at most (LDS list)

struct NuGenConst { double sigma_sq, rou_0, H; };

#pragma clang fp contract(off)
// the reference's is_point_inside_triangle(a, b, c, d)
__device__ __forceinline__ double nugen_cross(double ax, double ay, double bx, double by, double cx, double cy) {
    return (ax - cx) * (by - cy) - (bx - cx) * (ay - cy);
}
__device__ __forceinline__ bool nugen_inside(double px, double py, const double (&q)[6]) {
    const double d1 = nugen_cross(px, py, q[0], q[1], q[2], q[3]);
    const double d2 = nugen_cross(px, py, q[2], q[3], q[4], q[5]);
    const double d3 = nugen_cross(px, py, q[4], q[5], q[0], q[1]);
    const bool neg = (d1 < 0.0) || (d2 < 0.0) || (d3 < 0.0);
    const bool pos = (d1 > 0.0) || (d2 > 0.0) || (d3 > 0.0);
    return !(neg && pos);
}

// scan region of a sample: columns [x0, x0 + w), rows [y0, y0 + h) of the grid (w * h == 0: nothing to scan)
__device__ __forceinline__ void nugen_region(const double (&q)[6], int& x0, int& y0, int& w, int& h) {
    bool exact = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) exact = exact && q[k] == floor(q[k]) && fabs(q[k]) <= 1048576.0;
    if (exact && nugen_cross(q[0], q[1], q[2], q[3], q[4], q[5]) != 0.0) {
        const double lx = fmax(0.0, fmin(q[0], fmin(q[2], q[4]))), hx = fmin(400.0, fmax(q[0], fmax(q[2], q[4])));
        const double ly = fmax(0.0, fmin(q[1], fmin(q[3], q[5]))), hy = fmin(400.0, fmax(q[1], fmax(q[3], q[5])));
        x0 = (int)lx; y0 = (int)ly;
        w = hx >= lx ? (int)(hx - lx) + 1 : 0;
        h = hy >= ly ? (int)(hy - ly) + 1 : 0;
    } else {
        x0 = 0; y0 = 0; w = kNuGrid; h = kNuGrid;
    }
}

// per-point constants: rank[u], h^2 of the rank-0 user, D_1, D_2 (fs rows 0..2 are read: nfs >= 3)
__device__ __forceinline__ void nugen_point(int p, const double (&q)[6], const double* __restrict__ fs, const NuGenConst cc,
                                            int (&rank)[3], double& a, double& D1, double& D2) {
    const double px = (double)(p % kNuGrid), py = (double)(p / kNuGrid);
    const double HH = cc.H * cc.H;
    double hv[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const double dx = px - q[2 * u], dy = py - q[2 * u + 1];
        hv[u] = sqrt(cc.rou_0 / (HH + dx * dx + dy * dy));
    }
    int order[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        int r = 0;
#pragma unroll
        for (int v = 0; v < 3; ++v) r += (hv[v] > hv[u] || (hv[v] == hv[u] && v < u)) ? 1 : 0;
        rank[u] = r;
    }
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        if (rank[u] == 0) order[0] = u;
        if (rank[u] == 1) order[1] = u;
        if (rank[u] == 2) order[2] = u;
    }
    double S = 0.0;
#pragma unroll
    for (int u = 0; u < 3; ++u) S += fs[3 * order[0] + rank[u]];
    D1 = S + cc.sigma_sq / (hv[order[1]] * hv[order[1]]);
#pragma unroll
    for (int u = 0; u < 3; ++u) S += fs[3 * order[1] + rank[u]];
    D2 = S + cc.sigma_sq / (hv[order[2]] * hv[order[2]]);
    a = hv[order[0]] * hv[order[0]];
}

__device__ __forceinline__ bool nugen_better(double r, unsigned long long k, double br, unsigned long long bk) {
    return r > br || (r == br && k < bk);
}

// pass 1: grid = rows_in_chunk * tiles workgroups of kNuThreads; best_rate / best_key [rows_in_chunk][tiles]
__global__ __launch_bounds__(kNuThreads) void k_nu_tiles(const double* __restrict__ qs, const double* __restrict__ fs, int nfs,
                                                         const NuGenConst cc, int tile_pts, int tiles,
                                                         double* __restrict__ best_rate, unsigned long long* __restrict__ best_key) {
    __shared__ int s_list[kNuMaxTile];
    __shared__ int s_cnt;
    __shared__ double s_rate[kNuThreads];
    __shared__ unsigned long long s_key[kNuThreads];
    const int tid = threadIdx.x;
    const long long sample = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x % tiles);
    double q[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) q[k] = qs[sample * 6 + k];
    int x0, y0, w, h;
    nugen_region(q, x0, y0, w, h);
    const int start = tile * tile_pts;
    const int end = min(start + tile_pts, w * h);
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    for (int i = start + tid; i < end; i += kNuThreads) {
        const int x = x0 + i % w, y = y0 + i / w;
        if (nugen_inside((double)x, (double)y, q)) s_list[atomicAdd(&s_cnt, 1)] = y * kNuGrid + x;
    }
    __syncthreads();
    const int cnt = s_cnt;
    double br = -__builtin_inf();
    unsigned long long bk = ~0ull;
    for (int i = tid; i < cnt; i += kNuThreads) {
        const int p = s_list[i];
        int rank[3];
        double a, D1, D2;
        nugen_point(p, q, fs, cc, rank, a, D1, D2);
        // rate = (L_u0 + L_u1) + L_u2 with L_u the term of rank[u]; the first sum is commutative, so only the rank of user 2
        // (added last) decides the grouping
        const int last = rank[2];
        double pr = -__builtin_inf();
        int ps = 0;
        for (int s = 0; s < nfs; ++s) {
            const double l0 = log2(1.0 + fs[3 * s] * a / cc.sigma_sq);
            const double l1 = log2(1.0 + fs[3 * s + 1] / D1);
            const double l2 = log2(1.0 + fs[3 * s + 2] / D2);
            const double first = last == 0 ? l1 : l0;
            const double second = last == 2 ? l1 : l2;
            const double third = last == 0 ? l0 : (last == 1 ? l1 : l2);
            const double rate = (first + second) + third;
            if (rate > pr) { pr = rate; ps = s; }         // np.argmax: the first maximum
        }
        const unsigned long long key = ((unsigned long long)p << 32) | (unsigned)ps;
        if (nugen_better(pr, key, br, bk)) { br = pr; bk = key; }
    }
    s_rate[tid] = br; s_key[tid] = bk;
    __syncthreads();
    for (int o = kNuThreads / 2; o > 0; o >>= 1) {
        if (tid < o && nugen_better(s_rate[tid + o], s_key[tid + o], s_rate[tid], s_key[tid])) {
            s_rate[tid] = s_rate[tid + o]; s_key[tid] = s_key[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) { best_rate[blockIdx.x] = s_rate[0]; best_key[blockIdx.x] = s_key[0]; }
}

// pass 2: one workgroup per sample of the chunk; out [rows][6] = x, y, powers (user order), rate; zeros if nothing was inside
__global__ __launch_bounds__(kNuThreads) void k_nu_pick(const double* __restrict__ qs, const double* __restrict__ fs, const NuGenConst cc,
                                                        int tiles, const double* __restrict__ best_rate,
                                                        const unsigned long long* __restrict__ best_key, double* __restrict__ out) {
    __shared__ double s_rate[kNuThreads];
    __shared__ unsigned long long s_key[kNuThreads];
    const int tid = threadIdx.x;
    const long long sample = blockIdx.x;
    double br = -__builtin_inf();
    unsigned long long bk = ~0ull;
    for (int t = tid; t < tiles; t += kNuThreads) {
        const double r = best_rate[sample * tiles + t];
        const unsigned long long k = best_key[sample * tiles + t];
        if (nugen_better(r, k, br, bk)) { br = r; bk = k; }
    }
    s_rate[tid] = br; s_key[tid] = bk;
    __syncthreads();
    for (int o = kNuThreads / 2; o > 0; o >>= 1) {
        if (tid < o && nugen_better(s_rate[tid + o], s_key[tid + o], s_rate[tid], s_key[tid])) {
            s_rate[tid] = s_rate[tid + o]; s_key[tid] = s_key[tid + o];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    double* o = out + sample * 6;
    if (s_key[0] == ~0ull) {
        for (int k = 0; k < 6; ++k) o[k] = 0.0;
        return;
    }
    const int p = (int)(s_key[0] >> 32), s = (int)(s_key[0] & 0xffffffffull);
    double q[6];
    for (int k = 0; k < 6; ++k) q[k] = qs[sample * 6 + k];
    int rank[3];
    double a, D1, D2;
    nugen_point(p, q, fs, cc, rank, a, D1, D2);
    o[0] = (double)(p % kNuGrid);
    o[1] = (double)(p / kNuGrid);
    for (int u = 0; u < 3; ++u) o[2 + u] = fs[3 * s + rank[u]];
    o[5] = s_rate[0];
}
#pragma clang fp contract(fast)   // hipcc's default

}  // namespace dsg
