// Target-site LD (wld_run_targets): the rows of up to 16 chosen sites (a block
// of targets) against the 64 sites of one partner tile per 256-thread
// workgroup, every value exactly as the default row path (pair_valu_kernel<MF,
// REF>, pair_valu_kernel.hpp) computes the pair (min, max) — its operands (the
// lane-class layout), its f32 MFMA chains per lane class, its ordered
// horizontal sum, its scalar tail and ld_epilogue.
//
// Layout.  The A side is the block's target rows of the lane-class codes, read
// through the block's index list (an empty slot reads as an all-missing site);
// the B side the tile's 64 partner rows.  Wave w owns partners 16 w .. 16 w +
// 15 against the 16 targets: one 16x16 block of v_mfma_f32_16x16x4_f32, four
// accumulators (T, target-major x in, in x partner-major, both major).  Lane
// l = 16 g + r carries target r (A) / partner 16 w + r (B) at sequence kk + g
// and holds the sums of (target 4 g + e, partner 16 w + r), e = 0..3.
//
// Why a narrow kernel and not an instantiation of pair_valu_kernel: that
// template's workgroup is a 64x64 tile whose A rows are 64 consecutive sites
// dealt over four waves in up to four slots each (sixteen accumulators, the
// sub-block dealing, the row compaction); a rectangular 16 x 64 item with
// gathered A rows, one slot per wave and a dense output shares none of that,
// and threading an index list and a slot count through the template would put
// new branches into the row kernels' stage loop.  What must not drift — the
// order of the sums — is stated once there and restated here in the same
// terms (the class loop, acc_zero / compute_stage / acc_fold, the tail), and
// tests/test_gpu_targets.py compares the two paths bit for bit.
//
// Partners below the target.  With the target t on the A side the four sums
// are T = sum w [t in][s in], X1 = sum w [t major][s in], X2 = sum w [t in]
// [s major], AB = sum w [t major][s major]: each a chain, in the same sequence
// order, of terms that are w_k or 0 — the product u f is exact whichever
// factor carries the weight — so they are, bit for bit, the sums the row path
// forms for the pair with s on its A side.  For s > t the pair is (a, b) =
// (t, s): SA = X1, SB = X2.  For s < t it is (s, t): SA = X2, SB = X1.  The
// epilogue (not symmetric in SA, SB) then runs on the row path's arguments.
#include "pair_common.hpp"
#include "targets_plan.hpp"

namespace wld {

namespace {
constexpr int kTStride = 68;  // LDS row stride in bytes (17 dwords), as the row kernels'
typedef float t4f __attribute__((ext_vector_type(4)));
using targets_plan::kNoTarget;

__device__ inline void targets_guard(const TargetsLaunch &t, unsigned bit) { atomicOr(t.guard, bit); }
}  // namespace

__global__ __launch_bounds__(256) void targets_pair_kernel(TargetsLaunch t) {
    __shared__ __attribute__((aligned(16))) uint8_t sA[targets_plan::kBlock * kTStride];
    __shared__ __attribute__((aligned(16))) uint8_t sB[kTile * kTStride];
    __shared__ __attribute__((aligned(16))) float sW[64];
    __shared__ uint32_t sSite[targets_plan::kBlock];
    __shared__ uint32_t sPass[targets_plan::kBlock][4];  // per slot and wave: the wave's 16 pass bits

    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
    const uint32_t T = t.LP / kTile;
    // (the item and the sites it names come from device lists: each is checked
    // before anything is read or written through it)
    const uint32_t blk = t.items[2 * (size_t)blockIdx.x], tile = t.items[2 * (size_t)blockIdx.x + 1];
    if (blk >= t.n_blocks || tile >= T) {
        if (tid == 0) targets_guard(t, kTargetsGuardItem);
        return;
    }
    if (tid < targets_plan::kBlock) {
        uint32_t s = t.slot_site[(size_t)blk * targets_plan::kBlock + tid];
        if (s != kNoTarget && s >= t.L) {
            targets_guard(t, kTargetsGuardSite);
            s = kNoTarget;
        }
        sSite[tid] = s;
    }
    __syncthreads();
    const uint32_t b0 = tile * kTile;

    float tot[4][4];  // [e: target 4 g + e][sum]
    t4f acc[4];       // [sum], element e
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int q = 0; q < 4; ++q) tot[e][q] = 0.0f;

    // loaders: every thread 16 bytes of a partner row; threads 0..63 also of a
    // target row (an empty slot: zeros); threads 64..127 a weight
    const uint32_t lr = tid >> 2, part = tid & 3;
    const uint8_t *gB = t.rcodes + (size_t)(b0 + lr) * t.NPr + part * 16;  // (b0 + lr < LP)
    const uint32_t a_site = tid < 64 ? sSite[lr] : kNoTarget;
    const uint8_t *gA = a_site != kNoTarget ? t.rcodes + (size_t)a_site * t.NPr + part * 16 : nullptr;
    uint4 va = make_uint4(0, 0, 0, 0), vb;
    float wv = 0.0f;
    auto fetch_stage = [&](uint32_t k0) {
        vb = *reinterpret_cast<const uint4 *>(gB + k0);
        if (gA) va = *reinterpret_cast<const uint4 *>(gA + k0);
        if (tid >= 64 && tid < 128) wv = t.rw[k0 + tid - 64];
    };
    auto store_stage = [&]() {
        __syncthreads();
        uint32_t *pb = reinterpret_cast<uint32_t *>(sB + lr * kTStride + part * 16);
        pb[0] = vb.x, pb[1] = vb.y, pb[2] = vb.z, pb[3] = vb.w;
        if (tid < 64) {
            uint32_t *pa = reinterpret_cast<uint32_t *>(sA + lr * kTStride + part * 16);
            pa[0] = va.x, pa[1] = va.y, pa[2] = va.z, pa[3] = va.w;
        }
        if (tid >= 64 && tid < 128) sW[tid - 64] = wv;
        __syncthreads();
    };
    // the staged 64 positions in sequence order: transposed 16-position groups,
    // lane (r, g) reads the dword of its row at 16 grp + 4 g = elements 16 grp
    // + 4 e + g, e = 0..3 (pair_valu_kernel.hpp compute_stage, MF && REF)
    auto compute_stage = [&]() {
#pragma unroll
        for (int grp = 0; grp < 4; ++grp) {
            const float4 w4 = *reinterpret_cast<const float4 *>(sW + 16 * grp + 4 * g);
            const float we[4] = {w4.x, w4.y, w4.z, w4.w};
            const uint32_t a4 = *reinterpret_cast<const uint32_t *>(sA + r * kTStride + 4 * g + 16 * grp);
            const uint32_t b4 = *reinterpret_cast<const uint32_t *>(sB + (16 * wave + r) * kTStride + 4 * g + 16 * grp);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t ca = a4 >> (8 * e);
                const float u = (ca & kCodeIn) ? we[e] : 0.0f;
                const float v = (ca & kCodeMaj) ? we[e] : 0.0f;
                const float fi = (float)((b4 >> (8 * e)) & 1u), fm = (float)((b4 >> (8 * e + 1)) & 1u);
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(u, fi, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v, fi, acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(u, fm, acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(v, fm, acc[3], 0, 0, 0);
            }
        }
    };

    // the eight lane classes, each a chain from 0 folded into the ordered
    // horizontal sum, then the tail stage on that sum; the stages are
    // consecutive, each fetched while the one before is computed
    const uint32_t cls = 64 * t.ref_cs, n_cls = t.ref_cs ? 8u : 0u;
    const uint32_t end = n_cls * cls + (t.ref_tail_n ? 64u : 0u);  // (<= NPr)
    if (end) fetch_stage(0);
    for (uint32_t c = 0; c < n_cls; ++c) {
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = t4f{0.0f, 0.0f, 0.0f, 0.0f};
        for (uint32_t k0 = c * cls; k0 < (c + 1) * cls; k0 += 64) {
            store_stage();
            if (k0 + 64 < end) fetch_stage(k0 + 64);
            compute_stage();
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int q = 0; q < 4; ++q) tot[e][q] += acc[q][e];
    }
    if (t.ref_tail_n) {
        // the scalar tail (lib.rs:461-480): its <= 7 sequences added onto the
        // horizontal sums one by one, in order (fmaf(u, f, tot) = tot + u f
        // rounded once: u f is exact)
        store_stage();
        for (uint32_t k = 0; k < t.ref_tail_n; ++k) {
            const float we = sW[k];
            const uint32_t cb = sB[(16 * wave + r) * kTStride + k];
            const float fi = (float)(cb & 1u), fm = (float)(cb >> 1);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t ca = sA[(4 * g + e) * kTStride + k];
                const float u = (ca & kCodeIn) ? we : 0.0f;
                const float v = (ca & kCodeMaj) ? we : 0.0f;
                tot[e][0] = __builtin_fmaf(u, fi, tot[e][0]);
                tot[e][1] = __builtin_fmaf(v, fi, tot[e][1]);
                tot[e][2] = __builtin_fmaf(u, fm, tot[e][2]);
                tot[e][3] = __builtin_fmaf(v, fm, tot[e][3]);
            }
        }
    }

    // ---- epilogue: the pair (min, max) with the sums in its roles ----------
    const uint32_t s = b0 + 16 * wave + r;  // this lane's partner (< LP)
    const bool s_in = s < t.L;
    const bool s_ok = s_in && t.site_ok[s] != 0;
    const uint32_t hi_s = t.win_hi ? t.win_hi[s] : 0u;  // ([LP])
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t j = 4 * g + e, tg = sSite[j];
        const bool live = tg != kNoTarget && s_in && s != tg;
        const bool below = s < tg;  // the partner is the pair's a
        float d, dp, r2;
        ld_epilogue(tot[e][0], below ? tot[e][2] : tot[e][1], below ? tot[e][1] : tot[e][2], tot[e][3], d, dp, r2);
        bool pass = false;
        if (live) {
            const bool some = s_ok && t.site_ok[tg] != 0;
            const bool inw = !t.win_hi || (below ? tg <= hi_s : s <= t.win_hi[tg]);
            pass = some && inw && r2 > t.thr;  // lib.rs:660 strict '>' (NaN never passes)
            if (pass) {
                const size_t k = ((size_t)blk * targets_plan::kBlock + j) * t.LP + s;
                t.d[k] = d;
                t.dp[k] = dp;
                t.r2[k] = r2;
            }
        }
        const unsigned long long bal = __ballot(pass);
        if (r == 0) sPass[j][wave] = (uint32_t)(bal >> (16 * g)) & 0xFFFFu;
    }
    __syncthreads();
    if (tid < targets_plan::kBlock && sSite[tid] != kNoTarget) {
        unsigned long long m = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) m |= (unsigned long long)sPass[tid][w] << (16 * w);
        t.mask[((size_t)blk * targets_plan::kBlock + tid) * T + tile] = m;
    }
}

// One workgroup per slot: the slot's rows per tile as an exclusive prefix over
// its tiles (tile_pref) and their total (slot_cnt).
__global__ __launch_bounds__(256) void targets_count_kernel(TargetsLaunch t) {
    __shared__ uint32_t sw[4];
    const uint32_t T = t.LP / kTile, slot = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint32_t run = 0;
    for (uint32_t i0 = 0; i0 < T; i0 += 256) {
        const uint32_t i = i0 + tid;
        const uint32_t c = i < T ? (uint32_t)__popcll(t.mask[(size_t)slot * T + i]) : 0u;
        const uint32_t incl = wave_inclusive_scan(c);
        if (lane == 63) sw[wv] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            before += k < wv ? sw[k] : 0u;
            all += sw[k];
        }
        if (i < T) t.tile_pref[(size_t)slot * T + i] = run + before + incl - c;
        run += all;
        __syncthreads();
    }
    if (tid == 0) t.slot_cnt[slot] = run;
}

// One workgroup: the exclusive prefix of the slots' counts; slot_base[n] = the
// batch's rows.
__global__ __launch_bounds__(256) void targets_scan_kernel(TargetsLaunch t) {
    __shared__ uint32_t sw[4];
    const uint32_t n = t.n_blocks * targets_plan::kBlock, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint32_t run = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += 256) {
        const uint32_t i = i0 + tid;
        const uint32_t c = i < n ? t.slot_cnt[i] : 0u;
        const uint32_t incl = wave_inclusive_scan(c);
        if (lane == 63) sw[wv] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            before += k < wv ? sw[k] : 0u;
            all += sw[k];
        }
        if (i < n) t.slot_base[i] = run + before + incl - c;
        run += all;
        __syncthreads();
    }
    if (tid == 0) t.slot_base[n] = run;
}

// One wave per (slot, tile): the passing partners of the tile, ascending, at
// the slot's base plus the tile's prefix.  Parent indices from the resident
// site map.
__global__ __launch_bounds__(256) void targets_rows_kernel(TargetsLaunch t) {
    const uint32_t T = t.LP / kTile, lane = threadIdx.x & 63;
    const uint64_t wi = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t n = (uint64_t)t.n_blocks * targets_plan::kBlock * T;
    if (wi >= n) return;
    const uint32_t slot = (uint32_t)(wi / T), tile = (uint32_t)(wi % T);
    const unsigned long long m = t.mask[wi];
    if (!m) return;
    const uint32_t tg = t.slot_site[slot], s = tile * kTile + lane;
    if (!((m >> lane) & 1ull)) return;
    const uint64_t pos = (uint64_t)t.slot_base[slot] + t.tile_pref[wi] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    // (a row outside the slot's range, the buffers or the set is not written)
    if (tg >= t.L || s >= t.L || pos >= t.slot_base[slot + 1] || pos >= t.out_cap) {
        targets_guard(t, kTargetsGuardRow);
        return;
    }
    const size_t k = (size_t)slot * t.LP + s;
    t.out_target[pos] = t.slot_pos[slot];
    t.out_site_target[pos] = t.site_map ? t.site_map[tg] : tg;
    t.out_site_partner[pos] = t.site_map ? t.site_map[s] : s;
    t.out_d[pos] = t.d[k];
    t.out_dp[pos] = t.dp[k];
    t.out_r2[pos] = t.r2[k];
}

void launch_targets_pairs(const TargetsLaunch &t, hipStream_t s) {
    if (!t.n_items) return;
    hipLaunchKernelGGL(targets_pair_kernel, dim3(t.n_items), dim3(256), 0, s, t);
}

void launch_targets_count(const TargetsLaunch &t, hipStream_t s) {
    if (!t.n_blocks) return;
    hipLaunchKernelGGL(targets_count_kernel, dim3(t.n_blocks * targets_plan::kBlock), dim3(256), 0, s, t);
    hipLaunchKernelGGL(targets_scan_kernel, dim3(1), dim3(256), 0, s, t);
}

void launch_targets_rows(const TargetsLaunch &t, hipStream_t s) {
    const uint64_t waves = (uint64_t)t.n_blocks * targets_plan::kBlock * (t.LP / kTile);
    if (!waves) return;
    hipLaunchKernelGGL(targets_rows_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, t);
}

}  // namespace wld
