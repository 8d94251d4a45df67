// Host check of weightedld_amd/csrc/prune_plan.hpp (stand-alone; built plain
// and with -fsanitize=address,undefined by tests/test_prune_plan.py):
//   - rank_of / first_nan: ties to the lower index, -0.0 == 0.0, +-inf, NaN;
//   - greedy against a brute-force restatement written here;
//   - the round rule (decide) under random asynchronous schedules — a random
//     subset of vertices per step, each read a random mix of stale and fresh
//     states: the fixed point, tags included, must equal sequential greedy on
//     a few thousand random graphs and on path, star, clique and empty graphs.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <utility>
#include <vector>

#include "prune_plan.hpp"

using namespace wld::prune_plan;

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                     \
    do {                                     \
        if (!(cond)) {                       \
            if (++g_fail <= 20) {            \
                printf("FAIL %s: ", #cond);  \
                printf(__VA_ARGS__);         \
                printf("\n");                \
            }                                \
        }                                    \
    } while (0)

struct Graph {
    size_t n = 0;
    std::vector<uint32_t> a, b;
};

// sequential greedy, restated on an adjacency matrix (not the plan's CSR)
Pruned brute(const Graph &g, const std::vector<uint32_t> &rank) {
    std::vector<uint32_t> order(g.n);
    for (size_t v = 0; v < g.n; ++v) order[rank[v]] = (uint32_t)v;
    std::vector<uint8_t> adj(g.n * g.n, 0);
    for (size_t e = 0; e < g.a.size(); ++e) adj[g.a[e] * g.n + g.b[e]] = adj[g.b[e] * g.n + g.a[e]] = 1;
    Pruned p;
    p.keep.assign(g.n, 0);
    p.tag.assign(g.n, 0);
    for (uint32_t v : order) {
        bool have = false;
        uint32_t best = v;
        for (uint32_t u = 0; u < g.n; ++u)
            if (adj[v * g.n + u] && p.keep[u] && (!have || rank[u] < rank[best])) best = u, have = true;
        p.keep[v] = !have;
        p.tag[v] = best;
        p.n_kept += !have;
    }
    return p;
}

// the round rule to its fixed point under a random schedule
Pruned rounds(const Graph &g, const std::vector<uint32_t> &rank, std::mt19937 &rng, bool &ok) {
    const size_t n = g.n;
    std::vector<std::vector<uint32_t>> hp(n);  // the neighbours ranking before v
    for (size_t e = 0; e < g.a.size(); ++e) {
        const uint32_t a = g.a[e], b = g.b[e];
        if (rank[a] < rank[b]) hp[b].push_back(a);
        else hp[a].push_back(b);
    }
    std::vector<uint32_t> state(n, kUndecided), stale(n, kUndecided), seen;
    auto step = [&](uint32_t v, int fresh_pct) {
        if (state[v] != kUndecided) return;
        seen.clear();
        for (uint32_t u : hp[v]) seen.push_back((int)(rng() % 100) < fresh_pct ? state[u] : stale[u]);
        const uint32_t s = decide(seen.data(), seen.size());
        if (s != kUndecided) state[v] = s;  // final once set
    };
    const int fresh_pct = (int)(rng() % 101), pick_pct = 1 + (int)(rng() % 100);
    size_t open = n;
    for (size_t t = 0; open && t < n / 2 + 8; ++t) {
        open = 0;
        for (uint32_t v = 0; v < n; ++v) {
            if (state[v] == kUndecided && (int)(rng() % 100) < pick_pct) step(v, fresh_pct);
            open += state[v] == kUndecided;
        }
        if (rng() % 2) stale = state;  // what a late reader may still see
    }
    // synchronous rounds to the fixed point: each decides at least the
    // best-ranked undecided vertex, so n rounds always suffice
    size_t left = n, r = 0;
    for (; left && r <= n; ++r) {
        stale = state;
        for (uint32_t v = 0; v < n; ++v) step(v, 0);
        left = 0;
        for (uint32_t v = 0; v < n; ++v) left += state[v] == kUndecided;
    }
    ok = left == 0;
    Pruned p;
    p.keep.assign(n, 0);
    p.tag.assign(n, 0);
    for (uint32_t v = 0; v < n; ++v) {
        p.keep[v] = state[v] == kKept;
        p.n_kept += p.keep[v];
        p.tag[v] = v;
        if (state[v] != kRemoved) continue;
        bool have = false;
        for (uint32_t u : hp[v])
            if (state[u] == kKept && (!have || rank[u] < rank[p.tag[v]])) p.tag[v] = u, have = true;
        ok = ok && have;
    }
    return p;
}

bool same(const Pruned &x, const Pruned &y) { return x.keep == y.keep && x.tag == y.tag && x.n_kept == y.n_kept; }

std::vector<float> random_priority(size_t n, std::mt19937 &rng) {
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<float> p(n);
    const int levels = 1 + (int)(rng() % 12);  // few levels: many ties
    for (auto &x : p) {
        const unsigned k = rng() % 40;
        x = k == 0 ? inf : k == 1 ? -inf : k == 2 ? 0.0f : k == 3 ? -0.0f : (float)((int)(rng() % levels) - levels / 2) * 0.5f;
    }
    return p;
}

void check_graph(const Graph &g, const float *priority, std::mt19937 &rng, const char *what) {
    const std::vector<uint32_t> rank = rank_of(priority, g.n);
    const Pruned ref = brute(g, rank), got = greedy(g.n, g.a.data(), g.b.data(), g.a.size(), rank);
    CHECK(same(ref, got), "%s: greedy differs from the restatement (n %zu, m %zu)", what, g.n, g.a.size());
    for (int rep = 0; rep < 2; ++rep) {
        bool ok = false;
        const Pruned fix = rounds(g, rank, rng, ok);
        CHECK(ok, "%s: the rounds left a vertex undecided or a removed one without a kept entry", what);
        CHECK(same(ref, fix), "%s: the rounds' fixed point differs from greedy (n %zu, m %zu)", what, g.n, g.a.size());
    }
    // the result's own properties: independent, maximal, tags kept neighbours
    std::vector<uint8_t> has_kept(g.n, 0);
    for (size_t e = 0; e < g.a.size(); ++e) {
        CHECK(!(got.keep[g.a[e]] && got.keep[g.b[e]]), "%s: edge %zu joins two kept sites", what, e);
        has_kept[g.a[e]] |= got.keep[g.b[e]];
        has_kept[g.b[e]] |= got.keep[g.a[e]];
    }
    for (size_t v = 0; v < g.n; ++v) {
        CHECK(got.keep[v] || has_kept[v], "%s: removed site %zu has no kept neighbour", what, v);
        CHECK(got.keep[v] ? got.tag[v] == v : (got.keep[got.tag[v]] && rank[got.tag[v]] < rank[v]), "%s: tag[%zu]", what, v);
    }
}

Graph random_graph(std::mt19937 &rng) {
    Graph g;
    g.n = 1 + rng() % 200;
    const double dens[] = {0.0, 0.01, 0.05, 0.3, 0.9};
    const double p = dens[rng() % 5];
    const bool banded = rng() % 2;  // windowed LD: edges between near sites only
    const size_t band = 1 + rng() % 20;
    for (uint32_t a = 0; a < g.n; ++a)
        for (uint32_t b = a + 1; b < g.n && (!banded || b - a <= band); ++b)
            if ((double)(rng() % 1000000) < p * 1e6) g.a.push_back(a), g.b.push_back(b);
    return g;
}

void check_ranks() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    {  // null: index order
        const std::vector<uint32_t> r = rank_of(nullptr, 5);
        for (uint32_t i = 0; i < 5; ++i) CHECK(r[i] == i, "identity rank[%u] = %u", i, r[i]);
        CHECK(rank_of(nullptr, 0).empty(), "empty");
    }
    {  // larger first, ties to the lower index, -0.0 == 0.0, +-inf at the ends
        const float p[] = {1.0f, -inf, 0.0f, 3.0f, -0.0f, 1.0f, inf, 0.0f, inf};
        const uint32_t want[] = {3, 8, 5, 2, 6, 4, 0, 7, 1};
        const std::vector<uint32_t> r = rank_of(p, 9);
        for (uint32_t i = 0; i < 9; ++i) CHECK(r[i] == want[i], "rank[%u] = %u, want %u", i, r[i], want[i]);
        CHECK(first_nan(p, 9) == 9, "no NaN here");
    }
    {
        const float p[] = {1.0f, inf, nan, -inf, nan};
        CHECK(first_nan(p, 5) == 2, "first NaN at 2, got %zu", first_nan(p, 5));
        CHECK(first_nan(p, 2) == 2, "none in the first two");
        CHECK(first_nan(nullptr, 0) == 0, "empty");
    }
    {  // the round rule itself
        const uint32_t s[] = {kRemoved, kUndecided, kKept, kRemoved};
        CHECK(decide(s, 0) == kKept, "no entry: kept");
        CHECK(decide(s, 1) == kKept, "all removed: kept");
        CHECK(decide(s, 2) == kUndecided, "an undecided entry, none kept: stays");
        CHECK(decide(s, 3) == kRemoved, "a kept entry: removed");
        CHECK(decide(s + 3, 1) == kKept, "removed only");
    }
}

}  // namespace

int main() {
    std::mt19937 rng(0x9121);
    check_ranks();
    for (size_t n : {0, 1, 2, 3, 64, 65, 200}) {
        Graph path, star, clique, empty;
        path.n = star.n = clique.n = empty.n = n;
        for (uint32_t i = 0; i + 1 < n; ++i) path.a.push_back(i), path.b.push_back(i + 1);
        for (uint32_t i = 1; i < n; ++i) star.a.push_back(0), star.b.push_back(i);
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t j = i + 1; j < n; ++j) clique.a.push_back(i), clique.b.push_back(j);
        for (int rep = 0; rep < 3; ++rep) {
            const std::vector<float> pr = random_priority(n, rng);
            const float *p = rep ? pr.data() : nullptr;
            check_graph(path, p, rng, "path");
            check_graph(star, p, rng, "star");
            check_graph(clique, p, rng, "clique");
            check_graph(empty, p, rng, "empty");
        }
        // known answers in index order
        const std::vector<uint32_t> id = rank_of(nullptr, n);
        const Pruned pp = greedy(n, path.a.data(), path.b.data(), path.a.size(), id);
        for (uint32_t i = 0; i < n; ++i)
            CHECK(pp.keep[i] == (i % 2 == 0) && pp.tag[i] == (i % 2 ? i - 1 : i), "path: site %u", i);
        const Pruned ps = greedy(n, star.a.data(), star.b.data(), star.a.size(), id);
        for (uint32_t i = 0; i < n; ++i) CHECK(ps.keep[i] == (i == 0) && ps.tag[i] == 0, "star: site %u", i);
        CHECK(greedy(n, empty.a.data(), empty.b.data(), 0, id).n_kept == n, "empty: all kept");
    }
    for (int it = 0; it < 3000; ++it) {
        const Graph g = random_graph(rng);
        const std::vector<float> pr = random_priority(g.n, rng);
        check_graph(g, it % 4 ? pr.data() : nullptr, rng, "random");
    }
    if (g_fail) {
        printf("%d checks FAILED\n", g_fail);
        return 1;
    }
    printf("prune_plan: ranks, greedy and the round rule under random schedules on 3000 random graphs OK\n");
    return 0;
}
