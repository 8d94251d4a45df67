// Host-side pieces of the partitioned LD scores (capi.hip wld_run_annot_scores;
// the kernel's epilogue in pair_annot.hip reads the image and the mask built
// here): the validation of an annotation matrix, its padded device image with
// the zero-chunk mask, the self-term rule, how two results of disjoint chunk
// ranges (or of a device group's members) add up, and the reader of the CLI's
// annotation file.  Header-only and free of HIP types so the host test
// (tests/cpp/annot_plan_check.cpp) checks the same code.
#pragma once
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace wld {
namespace annot_plan {

constexpr uint32_t kMaxAnnot = 128;   // WLD_ANNOT_MAX
constexpr uint32_t kColChunk = 16;    // annotation columns per product (one MFMA's N)
constexpr uint32_t kSiteTile = 64;    // the pair kernel's tile side
constexpr uint32_t kSiteChunk = 256;  // the reference's chunk side

// The first non-finite value of an n_sites x n_annot row-major matrix in
// row-major order: ok, or its (site, column).
struct Check {
    bool ok = true;
    uint64_t site = 0;
    uint32_t column = 0;
};
inline Check validate(const float *annot, uint64_t n_sites, uint32_t n_annot) {
    Check c;
    for (uint64_t i = 0; i < n_sites; ++i)
        for (uint32_t k = 0; k < n_annot; ++k)
            if (!std::isfinite(annot[i * n_annot + k])) {
                c.ok = false;
                c.site = i;
                c.column = k;
                return c;
            }
    return c;
}

inline uint32_t padded_columns(uint32_t n_annot) { return (n_annot + kColChunk - 1) / kColChunk * kColChunk; }

// The device image: LP x CP floats, row-major [site * CP + c], CP =
// padded_columns(n_annot), zero for site >= n_sites and c >= n_annot (LP: the
// padded site count, a multiple of 64, >= n_sites); and one byte per (64-site
// tile, 16-column chunk), [tile * (CP / 16) + chunk]: 1 when every value of
// the image in it is zero (+0 or -0), which the epilogue then skips — the
// terms it drops are exact zeros.
struct Image {
    uint32_t CP = 0;
    std::vector<float> values;
    std::vector<uint8_t> zero;
};
inline Image build_image(const float *annot, uint64_t n_sites, uint32_t n_annot, uint64_t LP) {
    Image im;
    im.CP = padded_columns(n_annot);
    const uint32_t chunks = im.CP / kColChunk;
    im.values.assign((size_t)LP * im.CP, 0.0f);
    im.zero.assign((size_t)(LP / kSiteTile) * chunks, 1);
    for (uint64_t i = 0; i < n_sites && i < LP; ++i)
        for (uint32_t k = 0; k < n_annot; ++k) {
            const float v = annot[i * n_annot + k];
            im.values[(size_t)i * im.CP + k] = v;
            if (v != 0.0f) im.zero[(size_t)(i / kSiteTile) * chunks + k / kColChunk] = 0;
        }
    return im;
}

// Linear index of the diagonal chunk (row, row) of an n_sites set in the
// reference's triu order (kernels.hpp chunk_linear: rows descend).
inline uint64_t diagonal_chunk(uint64_t n_sites, uint64_t row) {
    const uint64_t n = (n_sites + kSiteChunk - 1) / kSiteChunk, rf = n - 1 - row;
    return rf * (rf + 1) / 2;
}
// WLD_ANNOT_SELF: site i takes its self term in a run over the linear chunks
// [lb, le) iff its diagonal chunk (i / 256, i / 256) is one of them (and the
// site has a major and a minor symbol: the caller's site_ok).
inline bool self_in_range(uint64_t n_sites, uint64_t site, uint64_t lb, uint64_t le) {
    if (site >= n_sites) return false;
    const uint64_t lin = diagonal_chunk(n_sites, site / kSiteChunk);
    return lb <= lin && lin < le;
}

// A result on the host: counts exact, sums f64.  score: n_sites * n_annot,
// [site * n_annot + c]; partners: n_sites.
struct Scores {
    uint64_t n_sites = 0;
    uint32_t n_annot = 0;
    int flags = 0;
    uint64_t pairs = 0, none_pairs = 0, nonfinite_pairs = 0, counted_pairs = 0, tiles = 0;
    double kernel_ms = 0.0;
    std::vector<double> score;
    std::vector<uint32_t> partners;
};
// into += from: counts, scores and tiles by addition, kernel_ms the larger.
// false (nothing changed) when n_sites, n_annot or flags differ.
inline bool merge(Scores &into, const Scores &from) {
    if (into.n_sites != from.n_sites || into.n_annot != from.n_annot || into.flags != from.flags) return false;
    if (into.score.size() != from.score.size() || into.partners.size() != from.partners.size()) return false;
    into.pairs += from.pairs;
    into.none_pairs += from.none_pairs;
    into.nonfinite_pairs += from.nonfinite_pairs;
    into.counted_pairs += from.counted_pairs;
    into.tiles += from.tiles;
    if (from.kernel_ms > into.kernel_ms) into.kernel_ms = from.kernel_ms;
    for (size_t i = 0; i < from.score.size(); ++i) into.score[i] += from.score[i];
    for (size_t i = 0; i < from.partners.size(); ++i) into.partners[i] += from.partners[i];
    return true;
}

// ---- the annotation file (the CLI's --annot-input) ------------------------
// TSV: a header "site<TAB>name1<TAB>...", 1..128 names, distinct and
// non-empty; then one row per site: a parent site index (decimal) and one
// finite number per name.  Lines end in \n or \r\n; an empty last line is
// ignored.  Errors name the 1-based line.
struct File {
    std::vector<std::string> names;
    std::vector<uint64_t> site;  // per row
    std::vector<uint32_t> line;  // per row: its 1-based line in the file
    std::vector<float> values;   // rows x names, row-major
};

inline std::vector<std::string> split_tabs(const std::string &s) {
    std::vector<std::string> f;
    size_t at = 0;
    for (;;) {
        const size_t e = s.find('\t', at);
        f.push_back(s.substr(at, e == std::string::npos ? std::string::npos : e - at));
        if (e == std::string::npos) break;
        at = e + 1;
    }
    return f;
}

// Parses the text of a file; false with err set on a format error.
inline bool parse_text(const std::string &text, File &out, std::string &err) {
    out = File{};
    char msg[256];
    size_t at = 0;
    uint32_t ln = 0;
    bool have_header = false;
    while (at < text.size()) {
        size_t e = text.find('\n', at);
        if (e == std::string::npos) e = text.size();
        std::string row = text.substr(at, e - at);
        at = e + 1;
        ++ln;
        if (!row.empty() && row.back() == '\r') row.pop_back();
        if (row.empty() && at >= text.size()) break;  // (an empty last line)
        const std::vector<std::string> f = split_tabs(row);
        if (!have_header) {
            if (f[0] != "site") {
                err = "line 1: the header must begin with \"site\"";
                return false;
            }
            if (f.size() < 2) {
                err = "line 1: the header names no annotation";
                return false;
            }
            if (f.size() - 1 > kMaxAnnot) {
                snprintf(msg, sizeof msg, "line 1: %zu annotation columns; at most %u", f.size() - 1, kMaxAnnot);
                err = msg;
                return false;
            }
            for (size_t k = 1; k < f.size(); ++k) {
                if (f[k].empty()) {
                    snprintf(msg, sizeof msg, "line 1: the name of column %zu is empty", k);
                    err = msg;
                    return false;
                }
                for (size_t j = 1; j < k; ++j)
                    if (f[j] == f[k]) {
                        err = "line 1: the name \"" + f[k] + "\" appears twice";
                        return false;
                    }
                out.names.push_back(f[k]);
            }
            have_header = true;
            continue;
        }
        if (f.size() != out.names.size() + 1) {
            snprintf(msg, sizeof msg, "line %u: %zu fields; the header has %zu", ln, f.size(), out.names.size() + 1);
            err = msg;
            return false;
        }
        if (f[0].empty() || f[0].find_first_not_of("0123456789") != std::string::npos || f[0].size() > 19) {
            snprintf(msg, sizeof msg, "line %u: the site \"%.40s\" is not a site index", ln, f[0].c_str());
            err = msg;
            return false;
        }
        out.site.push_back(strtoull(f[0].c_str(), nullptr, 10));
        out.line.push_back(ln);
        for (size_t k = 1; k < f.size(); ++k) {
            const char *s = f[k].c_str();
            char *end = nullptr;
            const float v = strtof(s, &end);  // (strtof skips leading white space: refused here)
            if (f[k].empty() || s[0] == ' ' || end == s || *end != '\0') {
                snprintf(msg, sizeof msg, "line %u: field %zu \"%.40s\" is not a number", ln, k + 1, s);
                err = msg;
                return false;
            }
            if (!std::isfinite(v)) {
                snprintf(msg, sizeof msg, "line %u: field %zu \"%.40s\" is not finite", ln, k + 1, s);
                err = msg;
                return false;
            }
            out.values.push_back(v);
        }
    }
    if (!have_header) {
        err = "line 1: the file has no header";
        return false;
    }
    return true;
}

// Reads and parses a file; false with err set when it cannot be read or on a
// format error.
inline bool read_file(const char *path, File &out, std::string &err) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        err = std::string("cannot read ") + path + ": " + strerror(errno);
        return false;
    }
    std::string text;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) {
        err = std::string("cannot read ") + path;
        return false;
    }
    return parse_text(text, out, err);
}

// The forward merge-join: loaded site i (parent index parent[i], in loaded
// order) takes the first unused row at or after the previous match whose site
// equals parent[i]; rows of other sites in between are skipped, repeated
// parent indices take their rows in order.  annot: n x names, row-major.
// false with err set where a loaded site finds no row.
inline bool join(const File &file, const uint64_t *parent, size_t n, std::vector<float> &annot, std::string &err) {
    const size_t C = file.names.size(), R = file.site.size();
    annot.assign(n * C, 0.0f);
    size_t at = 0;
    uint32_t after = 1;  // the line of the previous match (the header's before the first)
    for (size_t i = 0; i < n; ++i) {
        while (at < R && file.site[at] != parent[i]) ++at;
        if (at == R) {
            char msg[200];
            snprintf(msg, sizeof msg, "no row for site %llu (site of interest %zu) after line %u",
                     (unsigned long long)parent[i], i, after);
            err = msg;
            return false;
        }
        after = file.line[at];
        for (size_t k = 0; k < C; ++k) annot[i * C + k] = file.values[at * C + k];
        ++at;
    }
    return true;
}

}  // namespace annot_plan
}  // namespace wld
