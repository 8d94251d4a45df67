// LD pruning on the device (wld_run_prune): from the rows'
// (a, b) of a thresholded run, in loaded indices, the greedy r2-independent
// site set under a rank, with a tag per removed site.
//
//   degree / scan / fill   directed CSR: every edge stored once, at its
//                          lower-priority endpoint — hp[v] = the neighbours
//                          that rank before v (u32 atomics count the degrees,
//                          one workgroup scans them, per-vertex cursors fill)
//   decide                 one round of the parallel form of sequential greedy
//                          (Blelloch, Fineman, Shun 2012; prune_plan.hpp has
//                          the rule and the argument): one wave per vertex,
//                          the lanes read the states of hp[v] 64 at a time and
//                          a ballot decides.  States are read and written
//                          with relaxed agent-scope atomics (a plain store is
//                          not seen across XCDs within a launch); a state once
//                          set is final, so a stale read only delays a
//                          decision.  No workgroup ever waits on another: a
//                          launch sweeps its vertices a fixed number of times
//                          and counts what is still undecided; the host
//                          launches rounds until that count is 0.
//   tags                   per removed vertex the KEPT entry of hp[v] with the
//                          smallest rank; keep[] and the kept count.
//
// Every index read from the edge list or the CSR is checked against its bound
// before it is used; a refusal sets a bit in the guard word and the host fails
// the call.
#include <algorithm>

#include "kernels.hpp"
#include "prune_plan.hpp"

namespace wld {

using prune_plan::kKept;
using prune_plan::kRemoved;
using prune_plan::kUndecided;

namespace {

__device__ inline uint32_t load_state(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline void store_state(uint32_t *p, uint32_t s) {
    __hip_atomic_store(p, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the endpoint an edge is stored at (v, the later in the order) and the entry
// it stores (u); false: an index out of range (or a loop), refused
__device__ inline bool edge_ends(const PruneArgs &p, uint32_t e, uint32_t &v, uint32_t &u) {
    const uint32_t a = p.ea[e], b = p.eb[e];
    if (a >= p.L || b >= p.L || a == b) {
        atomicOr(p.guard, kPruneGuardEdge);
        return false;
    }
    const bool a_first = p.rank[a] < p.rank[b];
    v = a_first ? b : a;
    u = a_first ? a : b;
    return true;
}

__global__ __launch_bounds__(256) void prune_degree_kernel(PruneArgs p) {
    for (uint32_t e = blockIdx.x * 256 + threadIdx.x; e < p.m; e += gridDim.x * 256) {
        uint32_t v, u;
        if (edge_ends(p, e, v, u)) atomicAdd(&p.off[v + 1], 1u);
    }
}

// Inclusive scan in place of off[1..L] (off[0] = 0 already; the degrees were
// counted into off[v + 1]), one workgroup: a contiguous slice per thread, the
// 1024 slice sums scanned in LDS.  cur[v] = off[v], the fill's cursors.
__global__ __launch_bounds__(1024) void prune_scan_kernel(PruneArgs p) {
    __shared__ uint32_t part[1024];
    const uint32_t t = threadIdx.x, per = (p.L + 1023) / 1024;
    const uint32_t lo = min(p.L, t * per), hi = min(p.L, lo + per);
    uint32_t s = 0;
    for (uint32_t v = lo; v < hi; ++v) s += p.off[v + 1];
    part[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint32_t x = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    uint32_t run = part[t] - s;  // exclusive
    for (uint32_t v = lo; v < hi; ++v) {
        p.cur[v] = run;
        run += p.off[v + 1];
        p.off[v + 1] = run;
    }
}

__global__ __launch_bounds__(256) void prune_fill_kernel(PruneArgs p) {
    for (uint32_t e = blockIdx.x * 256 + threadIdx.x; e < p.m; e += gridDim.x * 256) {
        uint32_t v, u;
        if (!edge_ends(p, e, v, u)) continue;
        const uint32_t at = atomicAdd(&p.cur[v], 1u);
        if (at < p.off[v + 1] && at < p.m) p.hp[at] = u;
        else atomicOr(p.guard, kPruneGuardFill);
    }
}

// One round.  prev: the undecided count of the launch before (null: none
// known): at 0 the launch has nothing to do.  left: this launch's count,
// zero before it, taken in its last sweep.
__global__ __launch_bounds__(256) void prune_decide_kernel(PruneArgs p, const unsigned *prev, unsigned *left) {
    if (prev && __hip_atomic_load(prev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = gridDim.x * 4;
    uint32_t undecided = 0;
    for (uint32_t sweep = 0; sweep < kPruneSweeps; ++sweep) {
        undecided = 0;
        for (uint32_t v = wave; v < p.L; v += n_waves) {
            if (load_state(p.state + v) != kUndecided) continue;  // (wave-uniform: one address)
            const uint32_t b = p.off[v], e = p.off[v + 1];
            bool kept = false, open = false;
            if (e > p.m || b > e) {  // a broken list decides nothing
                if (lane == 0) atomicOr(p.guard, kPruneGuardList);
                ++undecided;
                continue;
            }
            // 64 entries at a time; a KEPT one ends the list, an undecided one
            // does not (a later slice may still hold a KEPT one)
            for (uint32_t i = b; i < e && !kept; i += 64) {
                uint32_t s = kRemoved;
                if (i + lane < e) {
                    const uint32_t u = p.hp[i + lane];
                    if (u < p.L) {
                        s = load_state(p.state + u);
                    } else {
                        s = kUndecided;
                        atomicOr(p.guard, kPruneGuardList);
                    }
                }
                kept = __ballot(s == kKept) != 0;
                open |= __ballot(s == kUndecided) != 0;
            }
            if (kept) {
                if (lane == 0) store_state(p.state + v, kRemoved);
            } else if (!open) {
                if (lane == 0) store_state(p.state + v, kKept);
            } else {
                ++undecided;
            }
        }
    }
    if (lane == 0 && undecided) atomicAdd(left, undecided);
}

__global__ __launch_bounds__(256) void prune_tags_kernel(PruneArgs p) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = gridDim.x * 4;
    uint32_t n_kept = 0;
    for (uint32_t v = wave; v < p.L; v += n_waves) {
        const uint32_t s = p.state[v];
        if (s == kKept) {
            if (lane == 0) {
                p.keep[v] = 1;
                p.tag[v] = v;
            }
            ++n_kept;
            continue;
        }
        const uint32_t b = p.off[v], e = p.off[v + 1];
        unsigned long long best = ~0ull;  // rank << 32 | vertex
        if (s == kRemoved && e <= p.m && b <= e)
            for (uint32_t i = b + lane; i < e; i += 64) {
                const uint32_t u = p.hp[i];
                if (u < p.L && p.state[u] == kKept) {
                    const unsigned long long key = (unsigned long long)p.rank[u] << 32 | u;
                    best = key < best ? key : best;
                }
            }
        for (int d = 32; d; d >>= 1) {
            const unsigned long long other = __shfl_xor(best, d);
            best = other < best ? other : best;
        }
        if (lane == 0) {
            p.keep[v] = 0;
            p.tag[v] = best == ~0ull ? v : (uint32_t)best;
            if (best == ~0ull) atomicOr(p.guard, kPruneGuardTag);  // undecided, or removed without a kept entry
        }
    }
    if (lane == 0 && n_kept) atomicAdd(p.n_kept, n_kept);
}

unsigned edge_grid(uint32_t m) { return (unsigned)std::min<uint32_t>((std::max<uint32_t>(m, 1) + 255) / 256, 4096); }
// four waves a workgroup, one vertex per wave at a time; at most 2048 workgroups
unsigned wave_grid(uint32_t L) { return (unsigned)std::min<uint32_t>((std::max<uint32_t>(L, 1) + 3) / 4, 2048); }

}  // namespace

void launch_prune_csr(const PruneArgs &p, hipStream_t s) {
    hipLaunchKernelGGL(prune_degree_kernel, dim3(edge_grid(p.m)), dim3(256), 0, s, p);
    hipLaunchKernelGGL(prune_scan_kernel, dim3(1), dim3(1024), 0, s, p);
    hipLaunchKernelGGL(prune_fill_kernel, dim3(edge_grid(p.m)), dim3(256), 0, s, p);
}

void launch_prune_decide(const PruneArgs &p, const unsigned *prev, unsigned *left, hipStream_t s) {
    hipLaunchKernelGGL(prune_decide_kernel, dim3(wave_grid(p.L)), dim3(256), 0, s, p, prev, left);
}

void launch_prune_tags(const PruneArgs &p, hipStream_t s) {
    hipLaunchKernelGGL(prune_tags_kernel, dim3(wave_grid(p.L)), dim3(256), 0, s, p);
}

}  // namespace wld
