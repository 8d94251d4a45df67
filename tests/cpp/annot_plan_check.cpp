// Host-only check of weightedld_amd/csrc/annot_plan.hpp against brute force:
// the validation's first non-finite index, the padded image and the
// zero-chunk mask, the self-term rule over every chunk range of 1..3 chunk
// rows, the merge, and the annotation-file reader with its merge-join on good
// and malformed files written here (argv[1]: a directory to write them in).
// Prints "OK" and exits 0 when everything agrees.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "annot_plan.hpp"

using namespace wld::annot_plan;

static int fails = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++fails;                                                  \
        }                                                             \
    } while (0)

static void check_validate() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
    std::vector<float> a(7 * 5, 0.5f);
    CHECK(validate(a.data(), 7, 5).ok);
    CHECK(validate(a.data(), 0, 5).ok);
    a[4 * 5 + 3] = nan;
    a[4 * 5 + 4] = inf;
    a[6 * 5 + 0] = -inf;
    Check c = validate(a.data(), 7, 5);
    CHECK(!c.ok && c.site == 4 && c.column == 3);
    a[2 * 5 + 4] = -inf;  // an earlier site, a later column: row-major order decides
    c = validate(a.data(), 7, 5);
    CHECK(!c.ok && c.site == 2 && c.column == 4);
    CHECK(validate(a.data(), 2, 5).ok);  // only the first two sites are read
    a.assign(35, std::numeric_limits<float>::max());
    a[0] = std::numeric_limits<float>::denorm_min();
    a[1] = -0.0f;
    CHECK(validate(a.data(), 7, 5).ok);
}

static void check_image() {
    std::mt19937 rng(0xA11);
    for (uint64_t L : {1, 63, 64, 65, 130})
        for (uint32_t C : {1, 15, 16, 17, 128})
            for (int kind = 0; kind < 3; ++kind) {
                const uint64_t LP = (L + 63) / 64 * 64 + (kind == 2 ? 64 : 0);  // (kind 2: a wholly padded tile)
                std::vector<float> a(L * C);
                for (uint64_t i = 0; i < L; ++i)
                    for (uint32_t k = 0; k < C; ++k) {
                        float v = (float)((int)(rng() % 17) - 8) / 4.0f;
                        if (kind >= 1 && (i / 64 + k / 16) % 2 == 0) v = (rng() % 5 == 0) ? -0.0f : 0.0f;  // zero blocks
                        if (kind == 1 && i == L - 1 && k == C - 1) v = 3.0f;
                        a[i * C + k] = v;
                    }
                const Image im = build_image(a.data(), L, C, LP);
                const uint32_t CP = (C + 15) / 16 * 16, chunks = CP / 16;
                CHECK(padded_columns(C) == CP && im.CP == CP && CP % 16 == 0 && CP >= C && CP < C + 16);
                CHECK(im.values.size() == LP * CP && im.zero.size() == LP / 64 * chunks);
                for (uint64_t i = 0; i < LP; ++i)
                    for (uint32_t k = 0; k < CP; ++k) {
                        const float want = (i < L && k < C) ? a[i * C + k] : 0.0f;
                        const float got = im.values[i * CP + k];
                        CHECK(got == want && std::signbit(got) == std::signbit(want));
                    }
                for (uint64_t t = 0; t < LP / 64; ++t)
                    for (uint32_t ch = 0; ch < chunks; ++ch) {
                        bool all_zero = true;  // brute force over the image itself
                        for (uint64_t i = 64 * t; i < 64 * t + 64; ++i)
                            for (uint32_t k = 16 * ch; k < 16 * ch + 16; ++k)
                                if (im.values[i * CP + k] != 0.0f) all_zero = false;
                        CHECK(im.zero[t * chunks + ch] == (all_zero ? 1 : 0));
                    }
            }
}

// the reference's triu order over n chunk rows: rows descend, columns ascend
static std::vector<std::pair<uint64_t, uint64_t>> chunk_sequence(uint64_t n) {
    std::vector<std::pair<uint64_t, uint64_t>> seq;
    for (uint64_t row = n; row-- > 0;)
        for (uint64_t col = row; col < n; ++col) seq.push_back({row, col});
    return seq;
}

static void check_self() {
    for (uint64_t L : {1, 2, 255, 256, 257, 300, 512, 513, 600, 768}) {
        const uint64_t n = (L + 255) / 256;
        const auto seq = chunk_sequence(n);
        CHECK(seq.size() == n * (n + 1) / 2);
        for (uint64_t row = 0; row < n; ++row) {
            const uint64_t d = diagonal_chunk(L, row);
            CHECK(d < seq.size() && seq[d].first == row && seq[d].second == row);
        }
        for (uint64_t lb = 0; lb <= seq.size(); ++lb)
            for (uint64_t le = lb; le <= seq.size() + 1; ++le)
                for (uint64_t i = 0; i < L + 2; i += (i % 256 == 255 || i % 256 == 0 || i + 3 > L) ? 1 : 51) {
                    bool want = false;
                    for (uint64_t q = lb; q < le && q < seq.size(); ++q)
                        if (i < L && seq[q].first == i / 256 && seq[q].second == i / 256) want = true;
                    CHECK(self_in_range(L, i, lb, le) == want);
                }
        // disjoint ranges that cover the sequence give every site its term exactly once
        for (uint64_t cut = 0; cut <= seq.size(); ++cut)
            for (uint64_t i = 0; i < L; i += 37)
                CHECK((int)self_in_range(L, i, 0, cut) + (int)self_in_range(L, i, cut, seq.size()) == 1);
    }
}

static Scores made(uint64_t L, uint32_t C, int flags, int seed) {
    Scores s;
    s.n_sites = L;
    s.n_annot = C;
    s.flags = flags;
    s.pairs = 100 + seed;
    s.none_pairs = 3 + seed;
    s.nonfinite_pairs = 1 + seed;
    s.counted_pairs = 96 - seed;
    s.tiles = 5 + seed;
    s.kernel_ms = 0.25 * (seed + 1);
    s.score.resize(L * C);
    s.partners.resize(L);
    for (size_t i = 0; i < s.score.size(); ++i) s.score[i] = 0.5 * (double)i - seed;
    for (size_t i = 0; i < L; ++i) s.partners[i] = (uint32_t)(i + seed);
    return s;
}

static void check_merge() {
    Scores a = made(5, 3, 1, 0);
    const Scores a0 = a, b = made(5, 3, 1, 2);
    CHECK(merge(a, b));
    CHECK(a.pairs == a0.pairs + b.pairs && a.none_pairs == a0.none_pairs + b.none_pairs);
    CHECK(a.nonfinite_pairs == a0.nonfinite_pairs + b.nonfinite_pairs && a.counted_pairs == a0.counted_pairs + b.counted_pairs);
    CHECK(a.tiles == a0.tiles + b.tiles && a.kernel_ms == b.kernel_ms);
    for (size_t i = 0; i < a.score.size(); ++i) CHECK(a.score[i] == a0.score[i] + b.score[i]);
    for (size_t i = 0; i < a.partners.size(); ++i) CHECK(a.partners[i] == a0.partners[i] + b.partners[i]);
    Scores c = made(5, 3, 1, 7);
    const Scores c0 = c;
    CHECK(merge(c, a0) && c.kernel_ms == c0.kernel_ms);  // the larger stays
    for (const Scores &bad : {made(4, 3, 1, 1), made(5, 2, 1, 1), made(5, 3, 0, 1)}) {
        Scores d = a0;
        CHECK(!merge(d, bad));
        CHECK(d.pairs == a0.pairs && d.score == a0.score && d.partners == a0.partners && d.tiles == a0.tiles);
    }
}

static bool parses(const std::string &text, File &f, std::string &err) { return parse_text(text, f, err); }

static void check_reader(const char *dir) {
    File f;
    std::string err;
    // a good file: rows of filtered-out sites, a repeated coordinate, CRLF, exponents, a last line without \n
    const std::string good = "site\tcoding\tmaf bin\n3\t1\t-0.5\r\n7\t0\t2e-3\n7\t1\t.25\n9\t-0\t1E2\n12\t5\t6";
    CHECK(parses(good, f, err));
    CHECK(f.names.size() == 2 && f.names[0] == "coding" && f.names[1] == "maf bin");
    CHECK(f.site == (std::vector<uint64_t>{3, 7, 7, 9, 12}) && f.line == (std::vector<uint32_t>{2, 3, 4, 5, 6}));
    CHECK(f.values == (std::vector<float>{1.f, -0.5f, 0.f, 2e-3f, 1.f, .25f, -0.f, 100.f, 5.f, 6.f}));
    std::vector<float> a;
    const uint64_t parent[] = {7, 7, 12};
    CHECK(join(f, parent, 3, a, err));
    CHECK(a == (std::vector<float>{0.f, 2e-3f, 1.f, .25f, 5.f, 6.f}));
    const uint64_t twice[] = {3, 3};  // a repeated coordinate with one row
    CHECK(!join(f, twice, 2, a, err) && err.find("site 3") != std::string::npos && err.find("line 2") != std::string::npos);
    const uint64_t back[] = {9, 7};  // rows are taken forwards only
    CHECK(!join(f, back, 2, a, err) && err.find("site 7") != std::string::npos);
    const uint64_t none[] = {4};
    CHECK(!join(f, none, 1, a, err) && err.find("site 4") != std::string::npos && err.find("line 1") != std::string::npos);
    CHECK(join(f, none, 0, a, err) && a.empty());
    // the file on disk, and one that is not there
    const std::string path = std::string(dir) + "/annot_good.tsv";
    FILE *o = fopen(path.c_str(), "wb");
    CHECK(o != nullptr);
    if (o) {
        fwrite(good.data(), 1, good.size(), o);
        fclose(o);
        File g;
        CHECK(read_file(path.c_str(), g, err) && g.site == f.site && g.values == f.values && g.names == f.names);
    }
    CHECK(!read_file((std::string(dir) + "/annot_absent.tsv").c_str(), f, err) && err.find("cannot read") != std::string::npos);
    // 128 names pass, 129 do not
    std::string head = "site";
    for (int k = 0; k < 128; ++k) head += "\tn" + std::to_string(k);
    CHECK(parses(head + "\n", f, err) && f.names.size() == 128 && f.site.empty());
    CHECK(!parses(head + "\textra\n", f, err) && err.find("129") != std::string::npos && err.find("line 1") != std::string::npos);
    struct Bad {
        const char *text, *says;
    };
    const Bad bads[] = {
        {"", "line 1"},                                  // empty
        {"pos\ta\n1\t2\n", "line 1"},                    // the header's first field
        {"site\n1\n", "line 1"},                         // no name
        {"site\ta\t\n1\t2\t3\n", "line 1"},              // an empty name
        {"site\ta\tb\ta\n", "appears twice"},            // a duplicate name
        {"site\ta\tb\n1\t2\n", "line 2"},                // a short row
        {"site\ta\tb\n1\t2\t3\n2\t3\t4\t5\n", "line 3"},  // a long row
        {"site\ta\n1\tx\n", "line 2"},                   // not a number
        {"site\ta\n1\t1.5x\n", "line 2"},                // trailing text
        {"site\ta\n1\t\n", "line 2"},                    // an empty field
        {"site\ta\n1\t 1\n", "line 2"},                  // white space
        {"site\ta\n1\t1\n2\tnan\n", "line 3"},           // not finite
        {"site\ta\n1\tinf\n", "not finite"},
        {"site\ta\n1\t1e99\n", "not finite"},            // overflows f32
        {"site\ta\n-1\t1\n", "line 2"},                  // not a site index
        {"site\ta\n1.0\t1\n", "line 2"},
        {"site\ta\n\t1\n", "line 2"},
        {"site\ta\n1\t1\n\n2\t2\n", "line 3"},           // an empty line inside
    };
    for (const Bad &b : bads) {
        err.clear();
        const bool ok = parses(b.text, f, err);
        if (ok || err.find(b.says) == std::string::npos) printf("text %s -> ok %d, \"%s\"\n", b.text, (int)ok, err.c_str());
        CHECK(!ok && err.find(b.says) != std::string::npos);
    }
}

int main(int argc, char **argv) {
    check_validate();
    check_image();
    check_self();
    check_merge();
    check_reader(argc > 1 ? argv[1] : ".");
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("OK\n");
    return 0;
}
