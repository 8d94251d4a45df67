// Host-side pieces of the LD summary (capi.hip wld_run_summary; the kernel's
// epilogue in pair_summary.hip uses the same bin index): which decay bin a
// pair's distance falls into, and how two summaries of disjoint chunk ranges
// (or of a device group's members) add up.  Header-only and free of HIP types
// so the host test (tests/cpp/summary_plan_check.cpp) checks the same code.
#pragma once
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define WLD_SUMMARY_HD __host__ __device__
#else
#define WLD_SUMMARY_HD
#endif

namespace wld {
namespace summary_plan {

constexpr uint32_t kMaxBins = 1024;

// The decay bin of a counted pair at distance dist = pos[b] - pos[a]:
// min(dist / bin_width, n_bins - 1) — the last bin also takes everything
// beyond it.  bin_width > 0, n_bins >= 1.  (Coordinates on the device are
// 32-bit: the 64-bit division is left to distances or widths that need it.)
WLD_SUMMARY_HD inline uint32_t bin_index(uint64_t dist, uint64_t bin_width, uint32_t n_bins) {
    const uint64_t q = ((dist | bin_width) >> 32) == 0 ? (uint64_t)((uint32_t)dist / (uint32_t)bin_width)
                                                        : dist / bin_width;
    return q < (uint64_t)(n_bins - 1) ? (uint32_t)q : n_bins - 1;
}

// A summary on the host: counts exact, sums f64.  score/partners have one
// entry per loaded site, the bin arrays n_bins entries (none without bins).
struct Summary {
    uint64_t pairs = 0, none_pairs = 0, nonfinite_pairs = 0, counted_pairs = 0;
    double r2_sum = 0.0;
    double kernel_ms = 0.0;
    std::vector<double> score;
    std::vector<uint32_t> partners;
    std::vector<uint64_t> bin_pairs;
    std::vector<double> bin_r2_sum;
};

// into += from: every count and sum element by element (the arrays of both
// have the same lengths; an empty `into` takes from's).  kernel_ms: the
// slower of the two (members of a device group run side by side).
inline void merge(Summary &into, const Summary &from) {
    into.pairs += from.pairs;
    into.none_pairs += from.none_pairs;
    into.nonfinite_pairs += from.nonfinite_pairs;
    into.counted_pairs += from.counted_pairs;
    into.r2_sum += from.r2_sum;
    if (from.kernel_ms > into.kernel_ms) into.kernel_ms = from.kernel_ms;
    if (into.score.size() < from.score.size()) into.score.resize(from.score.size(), 0.0);
    if (into.partners.size() < from.partners.size()) into.partners.resize(from.partners.size(), 0);
    if (into.bin_pairs.size() < from.bin_pairs.size()) into.bin_pairs.resize(from.bin_pairs.size(), 0);
    if (into.bin_r2_sum.size() < from.bin_r2_sum.size()) into.bin_r2_sum.resize(from.bin_r2_sum.size(), 0.0);
    for (size_t i = 0; i < from.score.size(); ++i) into.score[i] += from.score[i];
    for (size_t i = 0; i < from.partners.size(); ++i) into.partners[i] += from.partners[i];
    for (size_t i = 0; i < from.bin_pairs.size(); ++i) into.bin_pairs[i] += from.bin_pairs[i];
    for (size_t i = 0; i < from.bin_r2_sum.size(); ++i) into.bin_r2_sum[i] += from.bin_r2_sum[i];
}

}  // namespace summary_plan
}  // namespace wld
