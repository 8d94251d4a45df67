// The sweep scan on a band (wld_banded_pairsum_device, wld_banded_omega_device):
// the pair-sum table M[j][k] = sum of r2(u, v) over j <= u < v <= j + k in band
// storage, and per split of the alignment Kim and Nielsen's omega maximised
// over the flank borders, with Kelly's ZnS of the split's largest window.
//
// Every value is one fixed sequence of IEEE f64 operations (the build has
// -ffp-contract=off, and no multiply feeds an add), so the results equal the
// numpy twins bit for bit and two calls give identical bytes.  Only the
// counters (non-finite band elements, evaluated and skipped candidates) go
// through integer atomics.  No workgroup waits on another.
//
// pairsum_rows_kernel   P[j][k] = P[j][k-1] + b(j, k) in place in the table.  One
//                       wave per 64 rows; a 64 x 64 tile of the band is loaded
//                       as 64 row segments into LDS (f64, non-finite -> +0.0,
//                       column 0 and j + k >= n never read), lane r scans row
//                       r of the tile with its carry in a register, and the
//                       tile goes out as 64 row segments.
// pairsum_chains_kernel M[j][k] = M[j+1][k-1] + P[j][k] in place.  One wave per
//                       64 chains (end sites i0 .. i0 + 63): each step takes one
//                       row j, lane c its element k = i0 + c - j, so a step reads
//                       and writes one contiguous run of a row
//                       (banded_omega_plan::row_segment) and the chain's
//                       previous value stays in the lane's register; no LDS.
//                       Eight rows are loaded before their eight dependent adds.
//                       The tails (j + k >= n) are written +0.0 here.
// omega_check_kernel    lo <= c < hi < n and hi - lo <= K for every split; the
//                       first offender goes to a status word the host reads
//                       before it launches the scan.
// omega_scan_kernel     one workgroup per split.  A lane keeps a right border b
//                       (SR = M[c+1][b-c-1], r and r(r-1)/2 in registers), the
//                       four waves take the left borders a in turn (SL =
//                       M[a][c-a], one address for the wave), and ST = M[a][b-a]
//                       is read along row a: coalesced across the lanes.  Each
//                       lane keeps its best (omega, a, b) under the total order
//                       "larger omega, then smaller a, then smaller b"; shuffles
//                       and one LDS round finish the split.  Three f64 divisions
//                       per candidate, never a reciprocal.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "banded_omega_plan.hpp"
#include "kernels.hpp"

namespace wld {

namespace {
namespace bop = banded_omega_plan;
constexpr int kSide = 64;

template <typename TB>
__global__ __launch_bounds__(64) void pairsum_rows_kernel(BandedPairsumArgs a) {
    constexpr int S = kSide + 1;
    __shared__ double sT[kSide * S];
    const uint32_t lane = threadIdx.x, n = a.n, K = a.K;
    const uint64_t r0 = (uint64_t)blockIdx.x * kSide;
    const TB *__restrict__ B = reinterpret_cast<const TB *>(a.band);
    double *__restrict__ P = a.sums;
    const uint32_t tiles = bop::col_tiles(K);
    double carry = 0.0;
    unsigned long long bad = 0;
    for (uint32_t t = 0; t < tiles; ++t) {
        const uint64_t k = (uint64_t)t * kSide + lane;
#pragma unroll 8
        for (int rr = 0; rr < kSide; ++rr) {
            const uint64_t j = r0 + rr;
            const bool ok = j < n && k >= 1 && k <= K && j + k < n;
            double v = 0.0;
            if (ok) {
                v = (double)B[j * a.ld + k];
                if (!(fabs(v) <= 1.79769313486231570815e308)) {  // NaN or +-inf
                    v = 0.0;
                    ++bad;
                }
            }
            sT[rr * S + lane] = v;
        }
        __syncthreads();
#pragma unroll 8
        for (int s = 0; s < kSide; ++s) {
            carry = carry + sT[lane * S + s];
            sT[lane * S + s] = carry;
        }
        __syncthreads();
#pragma unroll 8
        for (int rr = 0; rr < kSide; ++rr) {
            const uint64_t j = r0 + rr;
            if (j < n && k <= K) P[j * a.lds + k] = sT[rr * S + lane];
        }
        __syncthreads();
    }
    if (bad) atomicAdd(a.nonfinite, bad);
}

__global__ __launch_bounds__(64) void pairsum_chains_kernel(BandedPairsumArgs a) {
    const uint32_t lane = threadIdx.x, n = a.n, K = a.K;
    const uint64_t i0 = (uint64_t)blockIdx.x * kSide, i = i0 + lane;
    double *M = a.sums;
    const bop::Rows rows = bop::rows(i0, n, K);
    if (rows.bottom > rows.top) return;
    const uint32_t cnt = rows.top - rows.bottom + 1;
    const bool live = i < n;  // (else the chain holds only +0.0 tails)
    double m = 0.0;
    for (uint32_t s0 = 0; s0 < cnt; s0 += 8) {
        double p[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t s = s0 + t;
            const uint64_t j = (uint64_t)rows.top - s;
            const bool ok = s < cnt && live && i > j && i - j <= K;  // (1 <= k <= K, j + k < n)
            p[t] = ok ? M[j * a.lds + (i - j)] : 0.0;
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t s = s0 + t;
            const uint64_t j = (uint64_t)rows.top - s;
            if (s < cnt && i >= j && i - j <= K) {
                if (live && i > j) m = m + p[t];
                M[j * a.lds + (i - j)] = live ? m : 0.0;
            }
        }
    }
}

__global__ __launch_bounds__(256) void omega_check_kernel(BandedOmegaArgs a) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= a.n_splits) return;
    if (!bop::split_ok(a.split[g], a.lo[g], a.hi[g], a.n, a.K)) atomicMin(a.status, (uint32_t)g);
}

struct Best {
    double w;
    uint32_t a, b;
};
// the total order of the candidates: larger omega, then smaller a, then
// smaller b; a = UINT32_MAX marks "none yet" and loses to every candidate
__device__ __forceinline__ bool better(double w, uint32_t ca, uint32_t cb, const Best &q) {
    if (q.a == 0xFFFFFFFFu) return true;
    return w > q.w || (w == q.w && (ca < q.a || (ca == q.a && cb < q.b)));
}

__global__ __launch_bounds__(256) void omega_scan_kernel(BandedOmegaArgs a, uint32_t g0) {
    __shared__ Best sBest[4];
    __shared__ unsigned long long sCnt[4][2];
    const uint32_t g = g0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t c = a.split[g], lo = a.lo[g], hi = a.hi[g];
    const double *__restrict__ M = a.sums;
    const size_t ld = a.lds;
    if (tid == 0) {
        const uint64_t w = (uint64_t)hi - lo + 1;
        a.zns[g] = M[(size_t)lo * ld + (hi - lo)] / (double)(w * (w - 1) / 2);
    }
    uint32_t nL, nR;
    bop::split_sides(c, lo, hi, a.min_side, &nL, &nR);
    Best best{0.0, 0xFFFFFFFFu, 0xFFFFFFFFu};
    unsigned long long ev = 0, sk = 0;
    if (nL && nR) {
        const uint32_t b_min = c + a.min_side;  // (<= hi: no wrap)
        const double *row_c = M + (size_t)(c + 1) * ld;
        for (uint32_t bc = lane; bc < nR; bc += 64) {
            const uint32_t b = b_min + bc;
            const uint64_t r = b - c;
            const double SR = row_c[b - c - 1];
            const uint64_t rr2 = r * (r - 1) / 2;
            for (uint32_t ai = wave; ai < nL; ai += 4) {
                const uint32_t aa = lo + ai;
                const uint64_t l = c - aa + 1;
                const double *row_a = M + (size_t)aa * ld;
                const double SL = row_a[c - aa], ST = row_a[b - aa];
                const double X = (ST - SL) - SR;
                const double t1 = (SL + SR) / (double)(l * (l - 1) / 2 + rr2);
                const double t2 = X / (double)(l * r) + a.eps;
                if (t2 > 0.0) {
                    ++ev;
                    const double w = t1 / t2;
                    if (better(w, aa, b, best)) best = Best{w, aa, b};
                } else {
                    ++sk;
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        Best o;
        o.w = __shfl_xor(best.w, off);
        o.a = __shfl_xor(best.a, off);
        o.b = __shfl_xor(best.b, off);
        if (o.a != 0xFFFFFFFFu && better(o.w, o.a, o.b, best)) best = o;
        ev += __shfl_xor(ev, off);
        sk += __shfl_xor(sk, off);
    }
    if (lane == 0) {
        sBest[wave] = best;
        sCnt[wave][0] = ev;
        sCnt[wave][1] = sk;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) {
            const Best o = sBest[w];
            if (o.a != 0xFFFFFFFFu && better(o.w, o.a, o.b, best)) best = o;
            ev += sCnt[w][0];
            sk += sCnt[w][1];
        }
        a.omega[g] = best.a == 0xFFFFFFFFu ? __builtin_nan("") : best.w;
        a.left[g] = best.a;
        a.right[g] = best.b;
        if (ev) atomicAdd(a.counts, ev);
        if (sk) atomicAdd(a.counts + 1, sk);
    }
}
}  // namespace

void launch_banded_pairsum(const BandedPairsumArgs &a, hipStream_t st) {
    if (!a.n) return;
    const dim3 rows(bop::row_blocks(a.n));
    if (a.band_f16) hipLaunchKernelGGL((pairsum_rows_kernel<_Float16>), rows, dim3(64), 0, st, a);
    else hipLaunchKernelGGL((pairsum_rows_kernel<float>), rows, dim3(64), 0, st, a);
    hipLaunchKernelGGL(pairsum_chains_kernel, dim3(bop::chain_blocks(a.n, a.K)), dim3(64), 0, st, a);
}

void launch_banded_omega_check(const BandedOmegaArgs &a, hipStream_t st) {
    if (!a.n_splits) return;
    hipLaunchKernelGGL(omega_check_kernel, dim3((uint32_t)(((uint64_t)a.n_splits + 255) / 256)), dim3(256), 0, st, a);
}

void launch_banded_omega(const BandedOmegaArgs &a, hipStream_t st) {
    constexpr uint32_t kMaxGrid = 1u << 30;
    for (uint64_t g0 = 0; g0 < a.n_splits; g0 += kMaxGrid)
        hipLaunchKernelGGL(omega_scan_kernel, dim3((uint32_t)std::min<uint64_t>(a.n_splits - g0, kMaxGrid)), dim3(256), 0,
                           st, a, (uint32_t)g0);
}

}  // namespace wld
