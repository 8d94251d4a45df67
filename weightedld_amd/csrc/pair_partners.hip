// Best partners (wld_run_partners): every considered pair's d, d' and r2
// exactly as the default row path computes them — pair_valu_kernel<MF, REF>'s
// operands, lane-class chains, ordered horizontal sum, scalar tail and
// ld_epilogue, instantiated from the one template in pair_valu_kernel.hpp —
// and, instead of rows, per site the best k candidates under the order of
// partners_plan.hpp.  A top-k list is not an atomic: no value goes through
// one.  Every tile writes its own parts of a staging buffer, and a merge kernel
// in which one wave owns a site folds the parts into the site's running list.
// The keys of a site are distinct, so the best k are one set whatever order
// the parts are met in: the result does not depend on scheduling, on the batch
// cut or on how the chunk range is split.
//
// The selecting epilogue.  After the sums, wave w's lane (r, g) holds tot[i][j]
// of the pairs (a = a0 + 16 w + 4 g + i, b = b0 + 16 j + r), i, j = 0..3.  A
// pair is considered when a < b < L and it is in the window; it is a candidate
// when also both sites have a statistic and r2 > thr (the row path's pass
// test).  The classes {pairs, none, passing} are counted with wave ballots, one
// global atomic per class and tile.
//   1. Every lane writes float_key(r2) of its candidates (0 otherwise) into a
//      128 x 64 LDS matrix: list al (0..63) is a row al's 64 b columns, list
//      64 + bl is b column bl's 64 a rows.  (16-byte granules are XOR-swizzled
//      by the list's low bits: the transposed writes would otherwise meet in
//      one bank.)
//   2. A wave takes 32 lists.  Lane l holds item l's key; a ballot gives the
//      list's candidates (none, the common case at a positive threshold: one
//      count written, nothing else).  Otherwise item l's rank is the number of
//      items before it in the order — a greater key, or an equal one at a
//      smaller index (= a smaller partner) — counted over 16 broadcast reads
//      of four keys, and written back in place of the key.  The count first
//      takes greater keys only (a compare and an add with carry per item);
//      two candidates with one key then share a rank, which shows when every
//      candidate writes its lane to its rank's slot and one of them does not
//      read itself back: only such a list is counted again with the tie rule.
//   3. Every lane reads the two ranks of each of its candidates and writes
//      {key, d, d'} (its own registers) straight to rank's slot of the a
//      row's part and of the b column's part, where the rank is below kp.
// A diagonal tile contributes a < b only; its sites receive a row part and a
// column part like any other tile's.
#include "pair_valu_kernel.hpp"
#include "partners_plan.hpp"

namespace wld {

namespace {
// LDS traffic between the lanes of one wave: the wave's earlier writes are
// visible to its later reads
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// word of item m in its swizzled list (sw = list & 15)
__device__ __forceinline__ uint32_t swz(uint32_t m, uint32_t sw) { return (((m >> 2) ^ sw) << 2) | (m & 3u); }
}  // namespace

__device__ __attribute__((always_inline)) void partners_epilogue(const PartnersArgs &p, const OrderArgs &o,
                                                                 const uint8_t *site_ok, uint32_t L, uint32_t a0,
                                                                 uint32_t b0, uint32_t tid, float thr,
                                                                 const float (&tot)[4][4][4]) {
    __shared__ __attribute__((aligned(16))) uint32_t sM[2 * kTile][kTile];  // keys, then ranks, per list
    __shared__ uint32_t sCls[3];  // pairs, none, passing of the tile
    __shared__ uint32_t sSlot[4][kTile];  // per wave: the lane that took a rank
    const uint32_t lane = tid & 63, wave = tid >> 6, g = lane >> 4, r = lane & 15;
    const uint32_t al0 = 16 * wave + 4 * g;  // this lane's a rows al0 + i; its b columns 16 j + r
    const uint32_t kp = p.kp;
    const size_t part0 = (size_t)blockIdx.x * (2 * kTile);  // the tile's first part
    if (tid < 3) sCls[tid] = 0;

    uint32_t inr = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t a = a0 + al0 + i, b = b0 + 16 * j + r;
            if ((a < b) & (b < L) & in_window(o, a, b)) inr |= 1u << (4 * i + j);
        }
    const uint32_t okA4 = *reinterpret_cast<const uint32_t *>(site_ok + a0 + al0);
    uint32_t okB = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) okB |= site_ok[b0 + 16 * j + r] ? 1u << j : 0u;
    __syncthreads();  // the class counts are zero

    // ---- 1: the values, the classes, the key matrix
    uint32_t n_pairs = 0, n_none = 0, n_pass = 0;  // of the wave (uniform)
    uint32_t cand = 0;                             // bit 4 i + j
    uint32_t key[4][4];
    float vd[4][4], vdp[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t bl = 16 * j + r;
        uint32_t colk[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float d, dp, r2;
            ld_epilogue(tot[i][j][0], tot[i][j][1], tot[i][j][2], tot[i][j][3], d, dp, r2);
            const bool in = (inr >> (4 * i + j)) & 1u;
            const bool some = ((okA4 >> (8 * i)) & 0xFFu) && ((okB >> j) & 1u);
            const bool pass = in && some && r2 > thr;  // lib.rs:660 strict '>'; NaN never passes
            n_pairs += (uint32_t)__popcll(__ballot(in));
            n_none += (uint32_t)__popcll(__ballot(in && !some));
            n_pass += (uint32_t)__popcll(__ballot(pass));
            if (pass) cand |= 1u << (4 * i + j);
            vd[i][j] = d;
            vdp[i][j] = dp;
            key[i][j] = heatmap_plan::float_key(r2);
            colk[i] = pass ? key[i][j] : 0u;
            sM[al0 + i][swz(bl, (al0 + i) & 15u)] = colk[i];
        }
        // the column list's four consecutive a rows: one granule
        *reinterpret_cast<uint4 *>(&sM[kTile + bl][swz(al0, bl & 15u)]) = make_uint4(colk[0], colk[1], colk[2], colk[3]);
    }
    if (lane == 0) {
        if (n_pairs) atomicAdd(&sCls[0], n_pairs);
        if (n_none) atomicAdd(&sCls[1], n_none);
        if (n_pass) atomicAdd(&sCls[2], n_pass);
    }
    __syncthreads();
    if (tid < 3 && sCls[tid]) atomicAdd(&p.classes[tid], (unsigned long long)sCls[tid]);

    // ---- 2: the ranks, 32 lists per wave
    for (uint32_t t = 0; t < 32; ++t) {
        const uint32_t list = 32 * wave + t, sw = list & 15u;
        const uint32_t kl = sM[list][swz(lane, sw)];
        const unsigned long long any = __ballot(kl != 0u);
        if (lane == 0) p.cnt[part0 + list] = min((uint32_t)__popcll(any), kp);
        if (!any) continue;  // (uniform)
        uint32_t rank = 0;
#pragma unroll
        for (uint32_t q = 0; q < 16; ++q) {
            const uint4 v = *reinterpret_cast<const uint4 *>(&sM[list][4 * q]);  // (broadcast)
            rank += v.x > kl;
            rank += v.y > kl;
            rank += v.z > kl;
            rank += v.w > kl;
        }
        if (kl != 0u) sSlot[wave][rank] = lane;  // (rank <= 63)
        wave_sync();
        const bool clash = kl != 0u && sSlot[wave][rank] != lane;
        if (__ballot(clash)) {  // (uniform) equal keys among the candidates: the whole order
            rank = 0;
#pragma unroll
            for (uint32_t q = 0; q < 16; ++q) {
                const uint4 v = *reinterpret_cast<const uint4 *>(&sM[list][4 * q]);
                const uint32_t m0 = 4 * (q ^ sw), km[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (uint32_t e = 0; e < 4; ++e) rank += (km[e] > kl) | ((km[e] == kl) & (m0 + e < lane));
            }
        }
        wave_sync();  // every lane has read the keys and its slot
        sM[list][swz(lane, sw)] = rank;
    }
    __syncthreads();

    // ---- 3: the selected candidates to their parts' slots
    if (!cand) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!((cand >> j) & 0x1111u)) continue;
        const uint32_t bl = 16 * j + r;
        const uint4 rc4 = *reinterpret_cast<const uint4 *>(&sM[kTile + bl][swz(al0, bl & 15u)]);
        const uint32_t rc[4] = {rc4.x, rc4.y, rc4.z, rc4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (!((cand >> (4 * i + j)) & 1u)) continue;
            const uint32_t al = al0 + i;
            const uint32_t rr = sM[al][swz(bl, al & 15u)];
            const uint32_t kd = __float_as_uint(vd[i][j]), kdp = __float_as_uint(vdp[i][j]);
            // {key low: 0xFFFFFFFF - partner, key high, d, d'}
            if (rr < kp)
                *reinterpret_cast<uint4 *>(&p.stage[(part0 + al) * kp + rr]) =
                    make_uint4(partners_plan::kNoPartner - (b0 + bl), key[i][j], kd, kdp);
            if (rc[i] < kp)
                *reinterpret_cast<uint4 *>(&p.stage[(part0 + kTile + bl) * kp + rc[i]]) =
                    make_uint4(partners_plan::kNoPartner - (a0 + al), key[i][j], kd, kdp);
        }
    }
}

// ---- the merge: four workgroups per 64-site block (16 sites each: enough
// waves to hide the loads), one wave per site (4 sites in turn).  Lane i holds entry i of the site's running list.  The block's
// parts are read 64 counts at a time; the non-empty ones are compacted (ballot)
// and taken 64 / kp parts at once, one entry per lane.  Every held entry's
// rank in the union (the running list and the new entries: distinct keys) is
// counted over the keys in LDS, the entries with rank < k go to slot rank, and
// lane i takes slot i back.  New entries below a full list's last key are
// dropped first, and a step without a survivor is skipped.  ent, the count and the block's CSR range are
// checked before anything is read through them.
__global__ __launch_bounds__(256) void partners_merge_kernel(PartnersMerge m) {
    __shared__ __attribute__((aligned(16))) unsigned long long sKey[4][2 * kTile];
    __shared__ __attribute__((aligned(16))) PartnerEntry sOut[4][kTile];
    __shared__ uint32_t sEnt[4][kTile], sCnt[4][kTile];
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6, blk = blockIdx.x >> 2, sub = blockIdx.x & 3u;
    if (blk >= m.n_blocks) return;
    const uint32_t e0 = m.csr_off[blk], e1 = m.csr_off[blk + 1];
    if (e0 > e1 || e1 > m.n_ent) {
        if (tid == 0) atomicOr(m.guard, kPartnersGuardEntry);
        return;
    }
    if (e0 == e1) return;
    const uint32_t kp = m.kp, k = m.k, per = kTile / kp;  // parts per step
    // (an entry in registers: {key low, key high, d, d'}, as the epilogue stores it)
    const uint4 none = make_uint4(0u, 0u, 0u, 0u);
    auto key_of = [](const uint4 &e) { return (unsigned long long)e.y << 32 | e.x; };
    const uint4 *stage = reinterpret_cast<const uint4 *>(m.stage);
    uint4 *run = reinterpret_cast<uint4 *>(m.run);
    uint4 *out = reinterpret_cast<uint4 *>(&sOut[w][0]);
    for (uint32_t s = 0; s < 4; ++s) {
        const uint32_t ls = 16 * sub + 4 * w + s, site = blk * kTile + ls;
        if (site >= m.L) break;  // (uniform)
        uint4 mine = none;
        if (lane < k) mine = run[(size_t)site * k + lane];
        bool changed = false;
        for (uint32_t base = e0; base < e1; base += kTile) {
            const uint32_t idx = base + lane;
            uint32_t ent = 0, c = 0;
            if (idx < e1) {
                ent = m.csr_ent[idx];
                if ((uint64_t)ent * kTile + ls >= m.n_parts) {
                    atomicOr(m.guard, kPartnersGuardEntry);
                } else {
                    c = m.cnt[(size_t)ent * kTile + ls];
                    if (c > kp) {
                        atomicOr(m.guard, kPartnersGuardPart);
                        c = 0;
                    }
                }
            }
            const unsigned long long mask = __ballot(c != 0u);
            if (!mask) continue;  // (uniform)
            const uint32_t nz = (uint32_t)__popcll(mask);
            wave_sync();  // (the step before has read sEnt, sCnt)
            if (c) {
                const uint32_t at = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
                sEnt[w][at] = ent;
                sCnt[w][at] = c;
            }
            wave_sync();
            for (uint32_t s0 = 0; s0 < nz; s0 += per) {
                const uint32_t pi = s0 + lane / kp, e = lane % kp;
                uint4 nw = none;
                if (lane < per * kp && pi < nz && e < sCnt[w][pi])
                    nw = stage[((size_t)sEnt[w][pi] * kTile + ls) * kp + e];
                // the floor: a full list's last key; a new entry below it cannot enter
                // (distinct keys; a list that is not full has key 0 there and drops nothing)
                const unsigned long long floor_key =
                    (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)mine.y, (int)(k - 1)) << 32 |
                    (uint32_t)__builtin_amdgcn_readlane((int)mine.x, (int)(k - 1));
                if (key_of(nw) <= floor_key) nw = none;
                const unsigned long long km = key_of(mine), kn = key_of(nw);
                if (!__ballot(kn != 0ull)) continue;  // (uniform)
                wave_sync();  // (the step before has read sKey, sOut)
                sKey[w][lane] = km;
                sKey[w][kTile + lane] = kn;
                out[lane] = none;
                wave_sync();
                uint32_t rank_m = 0, rank_n = 0;
                for (uint32_t q = 0; q < k; ++q) {  // (the running list: k slots)
                    const unsigned long long kq = sKey[w][q];
                    rank_m += kq > km;
                    rank_n += kq > kn;
                }
                for (uint32_t q = 0; q < per * kp; ++q) {
                    const unsigned long long kq = sKey[w][kTile + q];
                    rank_m += kq > km;
                    rank_n += kq > kn;
                }
                if (km && rank_m < k) out[rank_m] = mine;
                if (kn && rank_n < k) out[rank_n] = nw;
                wave_sync();
                mine = out[lane < k ? lane : 0];
                if (lane >= k) mine = none;
                changed = true;
            }
        }
        if (changed && lane < k) run[(size_t)site * k + lane] = mine;
    }
}

void launch_pair_partners(const ValuLaunch &v, const OrderArgs &o, const PartnersArgs &p, hipStream_t st) {
    if (!v.n_tiles) return;
    // one whole-tile workgroup per listed tile, as the summary and heat-map launches
    hipLaunchKernelGGL((pair_valu_kernel<false, false, true, true, false, kReducePartners>), dim3(v.n_tiles),
                       dim3(256), 0, st, v.codes, v.w, v.site_ok, v.tiles, v.n_tiles, (const unsigned *)nullptr,
                       (const uint32_t *)nullptr, (unsigned *)nullptr, (const unsigned *)nullptr, 0u, v.L, v.NP, 1u,
                       v.ref_cls / 64, v.ref_tail_n, v.n_chunk_rows, v.thr, o, p, ScanArgs{});
}

void launch_partners_merge(const PartnersMerge &m, hipStream_t st) {
    if (!m.n_blocks || !m.n_ent) return;
    hipLaunchKernelGGL(partners_merge_kernel, dim3(4 * m.n_blocks), dim3(256), 0, st, m);
}

}  // namespace wld
