// Host check of targets_plan.hpp against brute force: random monotone position
// maps with repeats, random windows (D, K) and random target lists.  Checks
// lo[], the partner ranges, the blocks and the permutation back to list
// positions, the item list, the batch cuts (a cap of exactly one block among
// them) and the position the validator names.  Prints OK.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

#include "targets_plan.hpp"
#include "window_plan.hpp"

using namespace wld;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAIL %s:%d: %s (case %d)\n", __FILE__, __LINE__, #c, g_case); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static int g_case = 0;

static bool in_window(const uint32_t *pos, uint32_t a, uint32_t b, uint64_t D, uint64_t K) {  // a < b
    const uint64_t pa = pos ? pos[a] : a, pb = pos ? pos[b] : b;
    return (D == 0 || pb - pa <= D) && (K == 0 || (uint64_t)(b - a) <= K);
}

static void check_validator(std::mt19937 &rng) {
    for (int it = 0; it < 400; ++it, ++g_case) {
        const uint32_t L = 1 + rng() % 40, n = rng() % 30;
        std::vector<uint32_t> t(n);
        for (auto &x : t) x = rng() % (L + (rng() % 4 == 0 ? 3 : 0));
        // brute force: the first position that is out of range or repeats an earlier one
        targets_plan::Bad want;
        for (uint32_t k = 0; k < n && want.kind == targets_plan::kFine; ++k) {
            if (t[k] >= L) want = {targets_plan::kOutOfRange, k, 0};
            else
                for (uint32_t j = 0; j < k; ++j)
                    if (t[j] == t[k]) {
                        want = {targets_plan::kRepeated, k, j};
                        break;
                    }
        }
        const targets_plan::Bad got = targets_plan::validate(t.data(), n, L);
        CHECK(got.kind == want.kind);
        if (want.kind != targets_plan::kFine) CHECK(got.pos == want.pos);
        if (want.kind == targets_plan::kRepeated) CHECK(got.first == want.first);
    }
    CHECK(targets_plan::validate(nullptr, 0, 0).kind == targets_plan::kFine);
}

static void check_plan(std::mt19937 &rng) {
    for (int it = 0; it < 600; ++it, ++g_case) {
        const uint32_t L = 1 + rng() % (it % 5 == 0 ? 700 : 200);
        const uint32_t LP = (L + 63) / 64 * 64, T = LP / 64;
        // a monotone position map with repeats (steps 0..3), or none
        std::vector<uint32_t> pos(L);
        uint32_t run = rng() % 5;
        for (auto &x : pos) x = (run += rng() % 4);
        const bool with_pos = rng() % 3 != 0;
        const uint64_t D = rng() % 3 == 0 ? 0 : rng() % 150, K = rng() % 3 == 0 ? 0 : rng() % 120;
        const bool windowed = D || K;
        const uint32_t *pp = with_pos ? pos.data() : nullptr;
        const std::vector<uint32_t> hi = windowed ? window_plan::limits(pp, L, D, K) : std::vector<uint32_t>();
        // a random list without repeats, any order
        std::vector<uint32_t> all(L);
        for (uint32_t i = 0; i < L; ++i) all[i] = i;
        std::shuffle(all.begin(), all.end(), rng);
        const uint32_t n = rng() % 4 == 0 ? L : rng() % (std::min<uint32_t>(L, 70) + 1);
        const std::vector<uint32_t> t(all.begin(), all.begin() + n);
        CHECK(targets_plan::validate(t.data(), n, L).kind == targets_plan::kFine);

        if (windowed) {  // lo: the first s with hi[s] >= t; partners exactly [lo, hi] \ {t}
            const std::vector<uint32_t> lo = targets_plan::lower_limits(hi);
            for (uint32_t x = 0; x < L; ++x) {
                uint32_t s = 0;
                while (hi[s] < x) ++s;
                CHECK(lo[x] == s);
                for (uint32_t y = 0; y < L; ++y) {
                    if (y == x) continue;
                    const bool in = in_window(pp, std::min(x, y), std::max(x, y), D, K);
                    CHECK(in == (y >= lo[x] && y <= hi[x]));
                }
            }
        }
        // the batch cap: exactly one block, a few blocks, everything, less than a block
        const uint64_t per_block = 16ull * LP;
        const uint64_t caps[] = {per_block, per_block * (1 + rng() % 4) + rng() % per_block, 1ull << 40, 1, per_block - 1};
        const uint64_t cap = caps[it % 5];
        const targets_plan::Plan p = targets_plan::make(t.data(), n, L, LP, hi, cap);
        CHECK(p.n_targets == n && p.n_blocks == (n + 15) / 16 && p.L == L);
        CHECK(p.slot_site.size() == (size_t)p.n_blocks * 16);
        // blocks: the targets in loaded order, 16 at a time; the permutation
        std::vector<uint32_t> sorted = t;
        std::sort(sorted.begin(), sorted.end());
        std::vector<char> seen(n, 0);
        for (size_t s = 0; s < p.slot_site.size(); ++s) {
            if (s >= n) {
                CHECK(p.slot_site[s] == targets_plan::kNoTarget && p.slot_pos[s] == targets_plan::kNoTarget);
                continue;
            }
            CHECK(p.slot_site[s] == sorted[s]);
            CHECK(p.slot_pos[s] < n && t[p.slot_pos[s]] == p.slot_site[s] && !seen[p.slot_pos[s]]);
            seen[p.slot_pos[s]] = 1;
            // the range against brute force
            const uint32_t x = p.slot_site[s];
            for (uint32_t y = 0; y < L; ++y) {
                if (y == x) continue;
                const bool in = !windowed || in_window(pp, std::min(x, y), std::max(x, y), D, K);
                CHECK(in == (y >= p.slot_lo[s] && y <= p.slot_hi[s]));
            }
            CHECK(p.slot_lo[s] <= x && x <= p.slot_hi[s]);
        }
        // items: (block, tile) where the tile holds an in-window partner of a target of the block
        CHECK(p.item_begin.size() == (size_t)p.n_blocks + 1 && p.item_begin[0] == 0);
        uint64_t n_items = 0;
        for (uint32_t b = 0; b < p.n_blocks; ++b) {
            std::vector<uint32_t> want;
            for (uint32_t tile = 0; tile < T; ++tile) {
                bool any = false;
                for (uint32_t j = 0; j < 16 && !any; ++j) {
                    const size_t s = (size_t)b * 16 + j;
                    if (s >= n) break;
                    const uint32_t x = p.slot_site[s];
                    for (uint32_t y = tile * 64; y < std::min(L, tile * 64 + 64) && !any; ++y)
                        any = y != x && (!windowed || in_window(pp, std::min(x, y), std::max(x, y), D, K));
                }
                if (any) want.push_back(tile);
            }
            const std::vector<uint32_t> got(p.item_tile.begin() + p.item_begin[b], p.item_tile.begin() + p.item_begin[b + 1]);
            CHECK(got == want);
            n_items += want.size();
        }
        CHECK(p.items() == n_items);
        // batches: consecutive, covering, each within the cap unless a single block
        if (!p.n_blocks) {
            CHECK(p.batches() == 0);
            continue;
        }
        CHECK(p.batch_begin.front() == 0 && p.batch_begin.back() == p.n_blocks);
        const uint64_t bb = std::max<uint64_t>(1, cap / per_block);
        std::multiset<std::pair<uint32_t, uint32_t>> launched;
        for (uint32_t k = 0; k < p.batches(); ++k) {
            const uint32_t b0 = p.batch_begin[k], b1 = p.batch_begin[k + 1];
            CHECK(b1 > b0);
            CHECK((b1 - b0) * per_block <= cap || b1 - b0 == 1);
            if (k + 1 < p.batches()) CHECK(b1 - b0 == bb);  // (greedy: every batch but the last is full)
            const std::vector<uint32_t> bi = targets_plan::batch_items(p, b0, b1);
            CHECK(bi.size() % 2 == 0);
            for (size_t i = 0; i < bi.size(); i += 2) {
                CHECK(bi[i] < b1 - b0 && bi[i + 1] < T);
                if (i) CHECK(bi[i - 1] < bi[i + 1] || (bi[i - 1] == bi[i + 1] && bi[i - 2] < bi[i]));  // tile-major
                launched.emplace(b0 + bi[i], bi[i + 1]);
            }
        }
        if (cap == per_block || cap < per_block) CHECK(p.batches() == p.n_blocks);
        std::multiset<std::pair<uint32_t, uint32_t>> planned;
        for (uint32_t b = 0; b < p.n_blocks; ++b)
            for (uint64_t i = p.item_begin[b]; i < p.item_begin[b + 1]; ++i) planned.emplace(b, p.item_tile[i]);
        CHECK(launched == planned);
    }
}

int main() {
    std::mt19937 rng(20241);
    check_validator(rng);
    check_plan(rng);
    // the own-tile rule at its corners: a target alone in the set, alone in its tile's range
    CHECK(!targets_plan::tile_has_partner(0, 0, 0, 0));
    CHECK(targets_plan::tile_has_partner(0, 0, 1, 0));
    CHECK(!targets_plan::tile_has_partner(64, 64, 200, 0));
    CHECK(!targets_plan::tile_has_partner(64, 10, 64, 1));
    CHECK(targets_plan::tile_has_partner(64, 10, 64, 0));
    std::printf("cases %d OK\n", g_case);
    return 0;
}
