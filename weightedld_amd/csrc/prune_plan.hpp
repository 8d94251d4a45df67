// Host-side pieces of LD pruning (capi.hip wld_run_prune; the kernels in
// prune.hip apply the same round rule with the same state codes): the rank of
// a priority, sequential greedy selection with tags on an edge list (the
// definition of the result), and the round rule whose fixed point the device
// reaches.  Header-only and free of HIP types so the host test
// (tests/cpp/prune_plan_check.cpp) checks the same code.
//
// The graph: vertices 0..n-1, undirected edges {a, b}.  The order: u comes
// before v iff rank[u] < rank[v] (ranks are a permutation of 0..n-1).  The
// result is the lexicographically first maximal independent set under that
// order: visit the vertices by rank, keep one iff no neighbour has been kept.
//
// Why rounds reach it (Blelloch, Fineman, Shun 2012): whether v is
// kept depends only on the neighbours that rank before it, hp(v).  The rule
// turns an undecided v into REMOVED once some u in hp(v) is KEPT, into KEPT
// once every u in hp(v) is REMOVED, and leaves it undecided otherwise; a state
// once set is never changed.  By induction over the rank every decision equals
// sequential greedy's: a KEPT read is final and greedy removes v for it; "all
// REMOVED" reads are final and greedy keeps v.  A stale read can only show
// UNDECIDED for a vertex that has been decided since, which delays v and never
// decides it differently — so any schedule, synchronous or not, ends at the
// same fixed point, and the best-ranked undecided vertex is decided by every
// round that visits it (everything in its hp is decided).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

namespace wld {
namespace prune_plan {

constexpr uint32_t kUndecided = 0, kKept = 1, kRemoved = 2;
// wld_run_prune refuses more edges (32-bit CSR offsets and cursors)
constexpr uint64_t kMaxEdges = 0x7FFFFFFFull;

// The first NaN of priority[0..n), or n.
inline size_t first_nan(const float *priority, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (std::isnan(priority[i])) return i;
    return n;
}

// rank[v] (0 = first) under: u before v iff priority[u] > priority[v], or
// they compare equal (-0.0 == 0.0) and u < v.  A null priority is index
// order.  The priorities hold no NaN (first_nan); +-inf order as floats do.
inline std::vector<uint32_t> rank_of(const float *priority, size_t n) {
    std::vector<uint32_t> order(n), rank(n);
    std::iota(order.begin(), order.end(), 0u);
    if (priority)
        std::stable_sort(order.begin(), order.end(),
                         [priority](uint32_t u, uint32_t v) { return priority[u] > priority[v]; });
    for (size_t k = 0; k < n; ++k) rank[order[k]] = (uint32_t)k;
    return rank;
}

struct Pruned {
    std::vector<uint8_t> keep;   // 1 kept, 0 removed
    std::vector<uint32_t> tag;   // v for a kept v; else its kept neighbour of the smallest rank
    uint64_t n_kept = 0;
};

// Undirected adjacency of an edge list as CSR (off has n + 1 entries).
inline void adjacency(size_t n, const uint32_t *ea, const uint32_t *eb, size_t m, std::vector<uint64_t> &off,
                      std::vector<uint32_t> &nbr) {
    off.assign(n + 1, 0);
    for (size_t e = 0; e < m; ++e) {
        ++off[ea[e] + 1];
        ++off[eb[e] + 1];
    }
    for (size_t v = 0; v < n; ++v) off[v + 1] += off[v];
    nbr.resize(2 * m);
    std::vector<uint64_t> cur(off.begin(), off.end() - 1);
    for (size_t e = 0; e < m; ++e) {
        nbr[cur[ea[e]]++] = eb[e];
        nbr[cur[eb[e]]++] = ea[e];
    }
}

// Sequential greedy selection with tags: the definition.
inline Pruned greedy(size_t n, const uint32_t *ea, const uint32_t *eb, size_t m, const std::vector<uint32_t> &rank) {
    std::vector<uint64_t> off;
    std::vector<uint32_t> nbr;
    adjacency(n, ea, eb, m, off, nbr);
    std::vector<uint32_t> order(n);
    for (size_t v = 0; v < n; ++v) order[rank[v]] = (uint32_t)v;
    Pruned p;
    p.keep.assign(n, 0);
    p.tag.resize(n);
    for (size_t k = 0; k < n; ++k) {
        const uint32_t v = order[k];
        // every kept neighbour so far ranks before v; the tag is the first of them
        uint32_t best = v;
        for (uint64_t i = off[v]; i < off[v + 1]; ++i) {
            const uint32_t u = nbr[i];
            if (p.keep[u] && (best == v || rank[u] < rank[best])) best = u;
        }
        p.keep[v] = best == v;
        p.tag[v] = best;
        p.n_kept += best == v;
    }
    return p;
}

// The round rule: the next state of an undecided vertex from the states read
// for hp(v), the neighbours that rank before it (count may be 0: kept).
inline uint32_t decide(const uint32_t *hp_states, size_t count) {
    bool undecided = false;
    for (size_t i = 0; i < count; ++i) {
        if (hp_states[i] == kKept) return kRemoved;
        undecided |= hp_states[i] == kUndecided;
    }
    return undecided ? kUndecided : kKept;
}

}  // namespace prune_plan
}  // namespace wld
