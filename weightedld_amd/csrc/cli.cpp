// weighted_ld — the reference CLI (rust/weighted_ld/src/main.rs) rebuilt on the
// C ABI of libweightedld.so.  Same flags (main.rs:14-68), same pipeline
// (main.rs:121-213), same TSV files (main.rs:70-119) and the same env_logger
// style log lines on stderr; the all-pairs step runs on the GPU.
//
// Additions (do not change the reference flags' meaning):
//   --vcf-input PATH   VCF input following WeightedLD.py's handle_vcf (no site
//                      filter, site index = POS), for BASELINE config 3
//   --device N         HIP device ordinal (default 0)
//   --devices G|LIST   shard the pair space over G devices (0..G-1) or a comma
//                      list of ordinals (repeats allowed) in this one process
//                      (wld_create_multi); overrides --device
//   --kernel K         auto | valu | mfma (default auto)
//   --max-distance D   only pairs at most D apart in parent coordinates (VCF
//   --max-sites K      POS, alignment columns) / at most K sites of interest
//                      apart (wld_set_window; a distance window needs a
//                      non-decreasing site map, else the library's message)
//   --ld-score-output FILE   per-site LD score TSV (site, partners, ld_score)
//   --decay-output FILE      r2 decay by distance TSV (bin_start, pairs, r2_sum,
//   --decay-bin-width W      mean_r2), W in parent coordinates, B bins (default
//   --decay-bins B           64; the last also takes every longer distance); one
//                      device summary pass over every in-window pair serves
//                      both files (wld_run_summary; no threshold applies)
//   --heatmap-output FILE    LD heat map TSV (cell_a_start, cell_b_start, pairs,
//   --heatmap-cell-width W   sum, mean, max): every in-window pair reduced on the
//   --heatmap-cell-sites S   device over a grid of cells — equal bins of W parent
//   --heatmap-region A:B     coordinates, or equal runs of S sites of interest
//   --heatmap-stat STAT      (exactly one of the two; at most 4,096 cells), of
//                      the whole set or of the sites with A <= coordinate < B;
//                      STAT r2 (default) or dprime (|D'|); cells without a pair
//                      are not written (wld_run_heatmap; no threshold applies)
//   --prune-output FILE      LD pruning TSV (site, kept, tag): the greedy set of
//   --prune-r2 T             sites no two of which have r2 > T (in the window),
//   --prune-priority P       visited by P = index (default) or maf (the larger
//                      minor-allele fraction first, ties to the lower index);
//                      tag: the kept site standing for a removed one
//                      (wld_run_prune; parent indices as in the pair TSV)
//   --ld-sites P[,P...]      target-site LD TSV (target, site, d, d', r2): the
//   --ld-sites-file FILE     rows of the sites at the given parent coordinates
//   --ld-sites-output FILE   (the list, then the file's, one per line; every
//   --ld-sites-r2 T          site of interest carrying a coordinate is a target)
//                      against every in-window partner with r2 > T (default:
//                      --r2-threshold's value), by target, then partner
//                      (wld_run_targets: targets x sites pairs, not the
//                      triangle); with it --pair-output may be left out
//   --partners-output FILE   best-partner TSV (site, partner, rank, d, d', r2):
//   --partners-k K           for every site of interest its K (1 to 64) strongest
//   --partners-r2 T          in-window partners with r2 > T (default:
//                      --r2-threshold's value), r2 descending then partner
//                      ascending, one line per (site, rank), rank from 0
//                      (wld_run_partners; parent indices as in the pair TSV);
//                      with it --pair-output may be left out
//   --matrix-output FILE     dense LD matrix (wld_run_matrix) of the sites of
//   --matrix-stat STAT       interest, or of those inside --matrix-region
//   --matrix-region A:B      START:END (parent coordinates): r (default), r2, d
//   --matrix-format FMT      or dprime; tsv (header row and first column =
//   --matrix-zero-missing    parent site indices, values %.9g) or npy (v1.0
//                      <f4, C order; the indices in FILE.sites); NaN entries
//                      become 0 (1 on the r / r2 diagonal) with
//                      --matrix-zero-missing; obeys --max-distance/--max-sites
//   --matrix-banded          with --matrix-format npy and a window: FILE holds
//                      the [n, K + 1] upper band of every site of interest
//                      (wld_run_matrix_banded; element [i, k] = entry (i, i + k),
//                      K the width the window needs) instead of the square
//   --omega-output FILE --omega-max-side S [--omega-grid G] [--omega-min-side M]
//   [--omega-max-distance D] [--omega-eps E]
//                      a selective-sweep scan (wld_run_omega): TSV position, left,
//                      right, omega, zns per split; sets the window to 2 S - 1 sites
//                      for the scan unless --max-sites is given
//   --annot-input FILE       partitioned LD scores (wld_run_annot_scores): FILE is
//   --annot-score-output FILE  a TSV "site<TAB>name1<TAB>..." of per-site
//   --annot-self             annotations by parent index; the output has site,
//                      partners and one <name>_l2 column per annotation;
//                      --annot-self also counts r2(i, i) = 1
//   --blocks-output FILE     LD-block TSV (block, first, last, sites, pairs,
//   --blocks-r2 T            informative, strong, mean, min): maximal runs of
//   --blocks-dprime T        consecutive sites of interest without a weak pair
//   --blocks-rule all|spine  (value < T; exactly one of r2 and the row path's
//   --blocks-min-sites M     |d'|) under the window, of at least M (default 2)
//                      sites; rule spine asks only a block's first and last
//                      site to have no weak pair inside it (wld_run_blocks;
//                      first/last as --prune-output prints sites); with it
//                      --pair-output may be left out
#include <chrono>
#include <cinttypes>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <thread>

#include <sys/ioctl.h>
#include <unistd.h>
#include <vector>

#include "weightedld.h"
#include "tsv_format.hpp"
#include "annot_plan.hpp"

namespace annot_plan = wld::annot_plan;

namespace {

int g_level = 3;  // 0 off, 1 error, 2 warn, 3 info, 4 debug, 5 trace

void init_logger() {
    const char *e = getenv("RUST_LOG");  // env_logger, default_filter_or("info") (main.rs:122)
    if (!e || !*e) return;
    std::string s(e);
    for (auto &c : s) c = (char)tolower(c);
    if (s.find("trace") != std::string::npos) g_level = 5;
    else if (s.find("debug") != std::string::npos) g_level = 4;
    else if (s.find("info") != std::string::npos) g_level = 3;
    else if (s.find("warn") != std::string::npos) g_level = 2;
    else if (s.find("error") != std::string::npos) g_level = 1;
    else if (s.find("off") != std::string::npos) g_level = 0;
}

void log_at(int level, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void log_at(int level, const char *fmt, ...) {
    if (level > g_level) return;
    static const char *names[] = {"", "ERROR", "WARN ", "INFO ", "DEBUG", "TRACE"};
    char ts[32];
    time_t t = time(nullptr);
    struct tm g;
    gmtime_r(&t, &g);
    strftime(ts, sizeof ts, "%Y-%m-%dT%H:%M:%SZ", &g);
    char msg[2048];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    fprintf(stderr, "[%s %s weighted_ld] %s\n", ts, names[level], msg);
}
#define INFO(...) log_at(3, __VA_ARGS__)

// Rust's Debug for std::time::Duration
std::string fmt_duration(std::chrono::nanoseconds d) {
    uint64_t ns = (uint64_t)d.count();
    auto frac = [](uint64_t whole, uint64_t rem, int digits, const char *unit) {
        char buf[64];
        if (rem == 0) {
            snprintf(buf, sizeof buf, "%" PRIu64 "%s", whole, unit);
        } else {
            char f[16];
            snprintf(f, sizeof f, "%0*" PRIu64, digits, rem);
            int n = (int)strlen(f);
            while (n > 0 && f[n - 1] == '0') f[--n] = 0;
            snprintf(buf, sizeof buf, "%" PRIu64 ".%s%s", whole, f, unit);
        }
        return std::string(buf);
    };
    if (ns >= 1000000000ull) return frac(ns / 1000000000ull, ns % 1000000000ull, 9, "s");
    if (ns >= 1000000ull) return frac(ns / 1000000ull, ns % 1000000ull, 6, "ms");
    if (ns >= 1000ull) return frac(ns / 1000ull, ns % 1000ull, 3, "\xC2\xB5s");
    return frac(ns, 0, 0, "ns");
}

// human_format::Formatter::new() (2 decimals, SI prefixes)
std::string human(double v, const char *units = "") {
    static const char *pre[] = {"", "K", "M", "G", "T", "P", "E", "Z", "Y"};
    int k = 0;
    double x = v;
    while (std::fabs(x) >= 1000.0 && k < 8) {
        x /= 1000.0;
        ++k;
    }
    char buf[64];
    snprintf(buf, sizeof buf, "%.2f %s%s", x, pre[k], units);
    return buf;
}

// indicatif 0.15's ProgressBar as main.rs sets it up (main.rs:89-97, 170-178):
// template "{spinner:.green} [{elapsed_precise}] [{wide_bar:.cyan/blue}]
// {percent}% ({per_sec} {eta_precise})", progress chars "#>-", drawn on stderr
// only when the log level enables info (log_enabled!(Level::Info)) and stderr
// is a terminal (indicatif's stderr target draws nothing otherwise), at most
// 15 frames a second; dropped unfinished, it clears its line.  So TSVs and
// log lines are byte-identical whether or not a bar was drawn.
// (WLD_FORCE_PROGRESS_BAR=1 draws on a non-terminal stderr too: the tests'
// hook, where no pseudo-terminal is available.)
class ProgressBar {
  public:
    explicit ProgressBar(uint64_t len)
        : len_(len), on_(g_level >= 3 && (isatty(2) || forced())), start_(std::chrono::steady_clock::now()),
          last_(start_) {}
    ~ProgressBar() {
        if (on_ && drawn_) fputs("\r\x1b[2K", stderr), fflush(stderr);
    }
    void set_position(uint64_t pos) {
        ++updates_;
        last_pos_ = pos;
        pos_ = std::min(pos, len_);
        if (!on_) return;
        const auto now = std::chrono::steady_clock::now();
        if (drawn_ && now - last_ < std::chrono::milliseconds(66)) return;  // indicatif's 15 Hz draw rate
        last_ = now;
        draw(now);
    }
    uint64_t updates() const { return updates_; }
    uint64_t last_position() const { return last_pos_; }

  private:
    static bool forced() {
        const char *e = getenv("WLD_FORCE_PROGRESS_BAR");
        return e && *e == '1';
    }
    static std::string hms(uint64_t secs) {
        char b[32];
        snprintf(b, sizeof b, "%02" PRIu64 ":%02" PRIu64 ":%02" PRIu64, secs / 3600, secs / 60 % 60, secs % 60);
        return b;
    }
    void draw(std::chrono::steady_clock::time_point now) {
        static const char *ticks[] = {"\u2801", "\u2802", "\u2804", "\u2840", "\u2880",
                                      "\u2820", "\u2810", "\u2808"};  // indicatif's default tick chars
        const double el = std::chrono::duration<double>(now - start_).count();
        const double frac = len_ ? (double)pos_ / (double)len_ : 1.0;
        const uint64_t per_sec = el > 0.0 ? (uint64_t)((double)pos_ / el) : 0;
        const uint64_t eta = pos_ && per_sec ? (uint64_t)((double)(len_ - pos_) / (double)per_sec) : 0;
        char tail[96];
        snprintf(tail, sizeof tail, "] %d%% (%" PRIu64 "/s %s)", (int)(frac * 100.0), per_sec, hms(eta).c_str());
        struct winsize ws{};
        const int cols = ioctl(2, TIOCGWINSZ, &ws) == 0 && ws.ws_col ? ws.ws_col : 80;
        const int width = std::max(1, cols - 14 - (int)strlen(tail));  // "T [hh:mm:ss] [" is 14 columns
        const int fill = std::min(width, (int)(frac * width));
        std::string done((size_t)fill, '#'), rest;
        if (fill < width) {
            done += '>';
            rest.assign((size_t)(width - fill - 1), '-');
        }
        fprintf(stderr, "\r\x1b[2K\x1b[32m%s\x1b[0m [%s] [\x1b[36m%s\x1b[34m%s\x1b[0m%s", ticks[tick_++ % 8],
                hms((uint64_t)el).c_str(), done.c_str(), rest.c_str(), tail);
        fflush(stderr);
        drawn_ = true;
    }
    uint64_t len_, pos_ = 0, last_pos_ = 0, updates_ = 0;
    bool on_, drawn_ = false;
    unsigned tick_ = 0;
    std::chrono::steady_clock::time_point start_, last_;
};

// The LD pass's progress_report closure (main.rs:184-188): pb.set_position
// per completed chunk, on the calling thread (wld_progress_fn)
void on_progress(uint64_t pairs_done, void *user) { static_cast<ProgressBar *>(user)->set_position(pairs_done); }

// Rust `{:.3}` of an f32 (main.rs:76,106): exact integer rounding, tsv_format.hpp
using wld_tsv::fmt3;
using wld_tsv::fmt_u64;

struct Opt {
    std::string fasta_input, vcf_input, weights_output, pair_output;
    float min_acgt = 0.8f, min_minor = 0.02f, max_minor = 0.5f, r2_threshold = 0.1f;
    bool unweighted = false;
    bool gpu_prepass = false;
    bool exact_sums = false;  // --exact-sums: WLD_OPT_REF_SUMS 0
    int device = 0;
    std::vector<int> devices;  // --devices: a multi-device context
    int kernel = WLD_KERNEL_AUTO;
    uint64_t max_distance = 0, max_sites = 0;  // --max-distance / --max-sites: wld_set_window (0: no limit)
    std::string ld_score_output, decay_output;  // --ld-score-output / --decay-output: wld_run_summary
    uint64_t decay_bin_width = 0, decay_bins = 64;
    // --heatmap-output / --heatmap-cell-width / --heatmap-cell-sites / --heatmap-region / --heatmap-stat: wld_run_heatmap
    std::string heatmap_output;
    uint64_t heatmap_cell_width = 0, heatmap_cell_sites = 0, heatmap_lo = 0, heatmap_hi = 0;
    bool have_heatmap_width = false, have_heatmap_sites = false, have_heatmap_region = false, have_heatmap_stat = false;
    int heatmap_stat = WLD_HEAT_R2;
    std::string prune_output;  // --prune-output / --prune-r2 / --prune-priority: wld_run_prune
    bool have_prune_r2 = false, prune_maf = false;
    float prune_r2 = 0.0f;
    // --ld-sites / --ld-sites-file / --ld-sites-output / --ld-sites-r2: wld_run_targets
    std::vector<uint64_t> ld_sites;
    std::string ld_sites_file, ld_sites_output;
    bool have_ld_sites = false, have_ld_sites_r2 = false;
    float ld_sites_r2 = 0.0f;
    // --partners-output / --partners-k / --partners-r2: wld_run_partners
    std::string partners_output;
    uint32_t partners_k = 0;
    bool have_partners_k = false, have_partners_r2 = false;
    float partners_r2 = 0.0f;
    // --blocks-output / --blocks-r2 / --blocks-dprime / --blocks-rule / --blocks-min-sites: wld_run_blocks
    std::string blocks_output;
    bool have_blocks_r2 = false, have_blocks_dprime = false, have_blocks_rule = false, have_blocks_min = false;
    float blocks_min_value = 0.0f;
    int blocks_rule = WLD_BLOCKS_ALL;
    uint32_t blocks_min_sites = 2;
    // --matrix-output / --matrix-stat / --matrix-region / --matrix-format / --matrix-zero-missing: wld_run_matrix
    std::string matrix_output;
    int matrix_stat = WLD_MATRIX_R;
    uint64_t matrix_lo = 0, matrix_hi = 0;
    bool have_matrix_stat = false, have_matrix_region = false, have_matrix_format = false, matrix_npy = false,
         matrix_zero_missing = false, matrix_banded = false;
    // --annot-input / --annot-score-output / --annot-self: wld_run_annot_scores
    std::string annot_input, annot_score_output;
    bool annot_self = false;
    // --omega-output / --omega-max-side / --omega-grid / --omega-min-side / --omega-max-distance / --omega-eps: wld_run_omega
    std::string omega_output;
    uint32_t omega_max_side = 0, omega_grid = 0, omega_min_side = 2;
    uint64_t omega_max_distance = 0;
    double omega_eps = 1e-5;
    bool have_omega_max_side = false;
    std::string omega_opt;  // the first --omega-* option given besides --omega-output
};

void usage(FILE *f) {
    fprintf(f,
            "weighted_ld 0.1.0\n"
            "A tool for computing sequence weighted linkage disequilibrium\n\n"
            "USAGE:\n    weighted_ld [FLAGS] [OPTIONS] --fasta-input <fasta-input> --pair-output <pair-output>\n\n"
            "FLAGS:\n"
            "    -h, --help          Prints help information\n"
            "        --unweighted    Use unit weights instead of Henikoff weights\n"
            "        --gpu-prepass   Filter sites and compute Henikoff weights on the GPU (FASTA input)\n"
            "        --exact-sums    (addition, not the reference's output) exact masked sums rounded once,\n"
            "                        instead of lib.rs's own f32 summation order; d' and r2 can differ from\n"
            "                        lib.rs's on rare-allele data (the default: output identical to the reference)\n"
            "        --annot-self    (addition) with --annot-score-output: every site with both symbols also counts\n"
            "                        r2 = 1 with itself, as LDSC's LD scores do\n"
            "    -V, --version       Prints version information\n\n"
            "OPTIONS:\n"
            "        --fasta-input <fasta-input>          The source file to load\n"
            "        --max-minor <max-minor>              Maximum fraction of minor symbols for a site to be considered "
            "[default: 0.5]\n"
            "        --min-acgt <min-acgt>                Minimum fractions of ACTG for a site to be considered "
            "[default: 0.8]\n"
            "        --min-minor <min-minor>              Minimum fraction of minor symbols for a site to be considered "
            "[default: 0.02]\n"
            "        --pair-output <pair-output>          Filename to write the per-pair weighted LD figures to, in Tab "
            "Separated Value format\n"
            "        --r2-threshold <r2-threshold>        Minimum value of R2 to be included in the output [default: "
            "0.1]\n"
            "        --weights-output <weights-output>    Filename to write the per-sequence weights to, in Tab "
            "Separated Value format\n"
            "        --vcf-input <vcf-input>              (addition) VCF input, WeightedLD.py handle_vcf semantics\n"
            "        --device <device>                    (addition) HIP device ordinal [default: 0]\n"
            "        --devices <devices>                  (addition) shard over G devices (0..G-1) or a list \"0,1,..\"\n"
            "        --kernel <kernel>                    (addition) auto | valu | mfma [default: auto]\n"
            "        --max-distance <max-distance>        (addition) only pairs at most this far apart in parent\n"
            "                                             coordinates (VCF POS, alignment columns) [default: no limit]\n"
            "        --max-sites <max-sites>              (addition) only pairs at most this many sites of interest\n"
            "                                             apart [default: no limit]\n"
            "        --ld-score-output <ld-score-output>  (addition) Filename to write the per-site LD scores to (site,\n"
            "                                             partners, ld_score: the sum of r2 with every in-window\n"
            "                                             partner, no threshold), in Tab Separated Value format\n"
            "        --decay-output <decay-output>        (addition) Filename to write the r2 decay by distance to\n"
            "                                             (bin_start, pairs, r2_sum, mean_r2); needs --decay-bin-width\n"
            "        --decay-bin-width <decay-bin-width>  (addition) width of a distance bin, in parent coordinates\n"
            "        --decay-bins <decay-bins>            (addition) number of bins, at most 1024; the last one also\n"
            "                                             takes every longer distance [default: 64]\n"
            "        --heatmap-output <heatmap-output>    (addition) Filename to write the LD heat map to (cell_a_start,\n"
            "                                             cell_b_start, pairs, sum, mean, max per cell with a pair);\n"
            "                                             needs one of --heatmap-cell-width, --heatmap-cell-sites;\n"
            "                                             obeys --max-distance, --max-sites and --devices\n"
            "        --heatmap-cell-width <heatmap-cell-width>  (addition) cells are equal bins of this many parent\n"
            "                                             coordinates (at most 4096 cells)\n"
            "        --heatmap-cell-sites <heatmap-cell-sites>  (addition) cells are equal runs of this many sites of\n"
            "                                             interest (at most 4096 cells)\n"
            "        --heatmap-region <heatmap-region>    (addition) \"START:END\": only the sites with START <=\n"
            "                                             coordinate < END [default: every site]\n"
            "        --heatmap-stat <heatmap-stat>        (addition) r2 | dprime (|D'|) [default: r2]\n"
            "        --prune-output <prune-output>        (addition) Filename to write the LD-pruned site set to (site,\n"
            "                                             kept, tag: the kept site that stands for a removed one);\n"
            "                                             needs --prune-r2; obeys --max-distance and --max-sites\n"
            "        --prune-r2 <prune-r2>                (addition) no two kept sites have r2 above this\n"
            "        --prune-priority <prune-priority>    (addition) index | maf: the order in which sites are kept\n"
            "                                             [default: index]\n"
            "        --ld-sites <ld-sites>                (addition) target sites: parent coordinates \"P[,P...]\";\n"
            "                                             every site of interest at one is a target\n"
            "        --ld-sites-file <ld-sites-file>      (addition) more target coordinates, one per line\n"
            "        --ld-sites-output <ld-sites-output>  (addition) Filename to write the targets' rows to (target,\n"
            "                                             site, d, d', r2: every in-window partner above the\n"
            "                                             threshold); --pair-output may then be left out\n"
            "        --ld-sites-r2 <ld-sites-r2>          (addition) Minimum value of R2 of a target row [default:\n"
            "                                             --r2-threshold's value]\n"
            "        --partners-output <partners-output>  (addition) Filename to write every site's best partners to\n"
            "                                             (site, partner, rank, d, d', r2); needs --partners-k;\n"
            "                                             obeys --max-distance, --max-sites and --devices;\n"
            "                                             --pair-output may then be left out\n"
            "        --partners-k <partners-k>            (addition) partners per site, 1 to 64\n"
            "        --partners-r2 <partners-r2>          (addition) Minimum value of R2 of a partner [default:\n"
            "                                             --r2-threshold's value]\n"
            "        --blocks-output <blocks-output>      (addition) Filename to write the LD blocks to (block, first,\n"
            "                                             last, sites, pairs, informative, strong, mean, min): runs\n"
            "                                             of consecutive sites without a weak pair; needs exactly one\n"
            "                                             of --blocks-r2 and --blocks-dprime; obeys --max-distance,\n"
            "                                             --max-sites and --devices; --pair-output may then be left out\n"
            "        --blocks-r2 <blocks-r2>              (addition) a pair is weak when its R2 is below this\n"
            "        --blocks-dprime <blocks-dprime>      (addition) a pair is weak when the row's |D'| is below this\n"
            "        --blocks-rule <blocks-rule>          (addition) all: no weak pair in a block; spine: none with its\n"
            "                                             first or last site [default: all]\n"
            "        --blocks-min-sites <blocks-min-sites>  (addition) smallest block reported, at least 2 [default: 2]\n"
            "        --matrix-output <matrix-output>      (addition) Filename to write the dense LD matrix of the sites\n"
            "                                             of interest to (symmetric; 0 outside the window; nan where a\n"
            "                                             pair has no value); obeys --max-distance, --max-sites\n"
            "        --matrix-stat <matrix-stat>          (addition) r (signed correlation) | r2 | d | dprime [default: r]\n"
            "        --matrix-region <matrix-region>      (addition) \"START:END\": only the sites with START <=\n"
            "                                             parent index < END\n"
            "        --matrix-format <matrix-format>      (addition) tsv (a header row and a first column of parent\n"
            "                                             site indices) | npy (float32; the indices go to\n"
            "                                             <matrix-output>.sites) [default: tsv]\n"
            "        --matrix-zero-missing                (addition) entries without a value become 0 (1 on the r / r2\n"
            "                                             diagonal)\n"
            "        --matrix-banded                      (addition) write the band of the windowed matrix instead of the\n"
            "                                             square: an [n, K+1] array, element [i, k] = entry (i, i+k), K\n"
            "                                             the width the window needs; needs --matrix-format npy and\n"
            "                                             --max-distance or --max-sites, takes no --matrix-region\n"
            "        --annot-input <annot-input>          (addition) per-site annotations, Tab Separated: a header\n"
            "                                             \"site<TAB>name1<TAB>...\" (1 to 128 names), then per site its\n"
            "                                             parent coordinate (as the pair output's site columns) and\n"
            "                                             one finite number per name; every site of interest needs a\n"
            "                                             row, in site order; needs --annot-score-output\n"
            "        --annot-score-output <annot-score-output>  (addition) Filename to write the partitioned LD scores\n"
            "                                             to (site, partners, <name>_l2 per annotation: the sum of r2\n"
            "                                             times the partner's annotation over every in-window partner,\n"
            "                                             no threshold); needs --annot-input; obeys --max-distance,\n"
            "                                             --max-sites and --devices; --pair-output may then be left out\n"
            "        --omega-output <omega-output>        (addition) Filename to write a selective-sweep scan to, Tab\n"
            "                                             Separated (position, left, right, omega, zns): per position\n"
            "                                             Kim and Nielsen's omega maximised over the flank borders,\n"
            "                                             the borders' parent coordinates (NA without a candidate) and\n"
            "                                             Kelly's ZnS of the largest window; omega and zns printed\n"
            "                                             with 17 significant digits; needs --omega-max-side; sets\n"
            "                                             the window to 2 * max-side - 1 sites unless --max-sites is\n"
            "                                             given; --pair-output may then be left out\n"
            "        --omega-max-side <omega-max-side>    (addition) the most sites a flank may hold\n"
            "        --omega-grid <omega-grid>            (addition) scan this many equidistant positions [default: 0,\n"
            "                                             every split between two sites of interest]\n"
            "        --omega-min-side <omega-min-side>    (addition) the fewest sites a flank may hold [default: 2]\n"
            "        --omega-max-distance <omega-max-distance>  (addition) a flank reaches at most this far from the\n"
            "                                             position, in parent coordinates [default: 0, no limit]\n"
            "        --omega-eps <omega-eps>              (addition) added to the cross term of omega [default: 1e-5]\n");
}

[[noreturn]] void arg_error(const char *msg, const char *arg) {
    fprintf(stderr, "error: %s '%s'\n\nUSAGE:\n    weighted_ld [FLAGS] [OPTIONS] --fasta-input <fasta-input> "
                    "--pair-output <pair-output>\n\nFor more information try --help\n", msg, arg);
    exit(1);
}

float parse_f32(const char *s, const char *name) {
    char *end = nullptr;
    float v = strtof(s, &end);
    if (!end || *end || !*s) {
        fprintf(stderr, "error: Invalid value for '--%s <%s>': invalid float literal\n", name, name);
        exit(1);
    }
    return v;
}

Opt parse(int argc, char **argv) {
    Opt o;
    bool have_pair = false;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i], val;
        bool has_eq = false;
        if (a.rfind("--", 0) == 0) {
            size_t eq = a.find('=');
            if (eq != std::string::npos) {
                val = a.substr(eq + 1);
                a = a.substr(0, eq);
                has_eq = true;
            }
        }
        auto need = [&](const char *name) -> std::string {
            if (has_eq) return val;
            if (i + 1 >= argc) arg_error("The argument requires a value but none was supplied:", name);
            return argv[++i];
        };
        if (a == "-h" || a == "--help") {
            usage(stdout);
            exit(0);
        } else if (a == "-V" || a == "--version") {
            printf("weighted_ld 0.1.0 (%s)\n", wld_version());
            exit(0);
        } else if (a == "--fasta-input") {
            o.fasta_input = need("--fasta-input");
        } else if (a == "--vcf-input") {
            o.vcf_input = need("--vcf-input");
        } else if (a == "--min-acgt") {
            o.min_acgt = parse_f32(need("--min-acgt").c_str(), "min-acgt");
        } else if (a == "--min-minor") {
            o.min_minor = parse_f32(need("--min-minor").c_str(), "min-minor");
        } else if (a == "--max-minor") {
            o.max_minor = parse_f32(need("--max-minor").c_str(), "max-minor");
        } else if (a == "--r2-threshold") {
            o.r2_threshold = parse_f32(need("--r2-threshold").c_str(), "r2-threshold");
        } else if (a == "--weights-output") {
            o.weights_output = need("--weights-output");
        } else if (a == "--pair-output") {
            o.pair_output = need("--pair-output");
            have_pair = true;
        } else if (a == "--unweighted") {
            o.unweighted = true;
        } else if (a == "--exact-sums") {
            o.exact_sums = true;
        } else if (a == "--gpu-prepass") {
            o.gpu_prepass = true;
        } else if (a == "--device") {
            o.device = atoi(need("--device").c_str());
        } else if (a == "--devices") {
            const std::string v = need("--devices");
            o.devices.clear();
            if (v.find(',') == std::string::npos) {
                const int g = atoi(v.c_str());
                if (g < 1) arg_error("Invalid value for '--devices':", v.c_str());
                for (int k = 0; k < g; ++k) o.devices.push_back(k);
            } else {
                size_t at = 0;
                while (at <= v.size()) {
                    const size_t e = std::min(v.find(',', at), v.size());
                    const std::string t = v.substr(at, e - at);
                    if (t.empty() || t.find_first_not_of("0123456789") != std::string::npos)
                        arg_error("Invalid value for '--devices':", v.c_str());
                    o.devices.push_back(atoi(t.c_str()));
                    at = e + 1;
                }
            }
        } else if (a == "--max-distance" || a == "--max-sites") {
            const std::string name = a, v = need(name.c_str());
            if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || v.size() > 19)
                arg_error(("Invalid value for '" + name + "':").c_str(), v.c_str());
            (name == "--max-distance" ? o.max_distance : o.max_sites) = strtoull(v.c_str(), nullptr, 10);
        } else if (a == "--ld-score-output") {
            o.ld_score_output = need("--ld-score-output");
        } else if (a == "--decay-output") {
            o.decay_output = need("--decay-output");
        } else if (a == "--decay-bin-width" || a == "--decay-bins") {
            const std::string name = a, v = need(name.c_str());
            if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || v.size() > 19)
                arg_error(("Invalid value for '" + name + "':").c_str(), v.c_str());
            (name == "--decay-bin-width" ? o.decay_bin_width : o.decay_bins) = strtoull(v.c_str(), nullptr, 10);
        } else if (a == "--heatmap-output") {
            o.heatmap_output = need("--heatmap-output");
        } else if (a == "--heatmap-cell-width" || a == "--heatmap-cell-sites") {
            const std::string name = a, v = need(name.c_str());
            if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || v.size() > 19 ||
                strtoull(v.c_str(), nullptr, 10) == 0)
                arg_error(("Invalid value for '" + name + "':").c_str(), v.c_str());
            (name == "--heatmap-cell-width" ? o.heatmap_cell_width : o.heatmap_cell_sites) = strtoull(v.c_str(), nullptr, 10);
            (name == "--heatmap-cell-width" ? o.have_heatmap_width : o.have_heatmap_sites) = true;
        } else if (a == "--heatmap-region") {
            const std::string v = need("--heatmap-region");
            const size_t c = v.find(':');
            const std::string lo = v.substr(0, std::min(c, v.size())), hi = c == std::string::npos ? "" : v.substr(c + 1);
            auto bad = [](const std::string &t) {
                return t.empty() || t.find_first_not_of("0123456789") != std::string::npos || t.size() > 19;
            };
            if (bad(lo) || bad(hi) || strtoull(lo.c_str(), nullptr, 10) > strtoull(hi.c_str(), nullptr, 10))
                arg_error("Invalid value for '--heatmap-region' (START:END):", v.c_str());
            o.heatmap_lo = strtoull(lo.c_str(), nullptr, 10);
            o.heatmap_hi = strtoull(hi.c_str(), nullptr, 10);
            o.have_heatmap_region = true;
        } else if (a == "--heatmap-stat") {
            const std::string k = need("--heatmap-stat");
            if (k != "r2" && k != "dprime") arg_error("Invalid value for '--heatmap-stat':", k.c_str());
            o.heatmap_stat = k == "dprime" ? WLD_HEAT_ABS_DPRIME : WLD_HEAT_R2;
            o.have_heatmap_stat = true;
        } else if (a == "--prune-output") {
            o.prune_output = need("--prune-output");
        } else if (a == "--prune-r2") {
            o.prune_r2 = parse_f32(need("--prune-r2").c_str(), "prune-r2");
            o.have_prune_r2 = true;
        } else if (a == "--prune-priority") {
            const std::string k = need("--prune-priority");
            if (k != "index" && k != "maf") arg_error("Invalid value for '--prune-priority':", k.c_str());
            o.prune_maf = k == "maf";
        } else if (a == "--ld-sites") {
            const std::string v = need("--ld-sites");
            o.have_ld_sites = true;
            size_t at = 0;
            while (at <= v.size()) {
                const size_t e = std::min(v.find(',', at), v.size());
                const std::string t = v.substr(at, e - at);
                if (t.empty() || t.find_first_not_of("0123456789") != std::string::npos || t.size() > 19)
                    arg_error("Invalid value for '--ld-sites':", v.c_str());
                o.ld_sites.push_back(strtoull(t.c_str(), nullptr, 10));
                at = e + 1;
            }
        } else if (a == "--ld-sites-file") {
            o.ld_sites_file = need("--ld-sites-file");
        } else if (a == "--ld-sites-output") {
            o.ld_sites_output = need("--ld-sites-output");
        } else if (a == "--ld-sites-r2") {
            o.ld_sites_r2 = parse_f32(need("--ld-sites-r2").c_str(), "ld-sites-r2");
            o.have_ld_sites_r2 = true;
        } else if (a == "--partners-output") {
            o.partners_output = need("--partners-output");
        } else if (a == "--partners-k") {
            const std::string v = need("--partners-k");
            if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || v.size() > 9 ||
                strtoull(v.c_str(), nullptr, 10) < 1 || strtoull(v.c_str(), nullptr, 10) > WLD_PARTNERS_MAX_K)
                arg_error("Invalid value for '--partners-k' (1 to 64):", v.c_str());
            o.partners_k = (uint32_t)strtoull(v.c_str(), nullptr, 10);
            o.have_partners_k = true;
        } else if (a == "--partners-r2") {
            o.partners_r2 = parse_f32(need("--partners-r2").c_str(), "partners-r2");
            o.have_partners_r2 = true;
        } else if (a == "--blocks-output") {
            o.blocks_output = need("--blocks-output");
        } else if (a == "--blocks-r2" || a == "--blocks-dprime") {
            const bool r2 = a == "--blocks-r2";
            o.blocks_min_value = parse_f32(need(a.c_str()).c_str(), r2 ? "blocks-r2" : "blocks-dprime");
            if (!std::isfinite(o.blocks_min_value))
                arg_error(r2 ? "Invalid value for '--blocks-r2' (a finite number):"
                             : "Invalid value for '--blocks-dprime' (a finite number):", argv[i]);
            (r2 ? o.have_blocks_r2 : o.have_blocks_dprime) = true;
        } else if (a == "--blocks-rule") {
            const std::string k = need("--blocks-rule");
            if (k != "all" && k != "spine") arg_error("Invalid value for '--blocks-rule':", k.c_str());
            o.blocks_rule = k == "spine" ? WLD_BLOCKS_SPINE : WLD_BLOCKS_ALL;
            o.have_blocks_rule = true;
        } else if (a == "--blocks-min-sites") {
            const std::string v = need("--blocks-min-sites");
            if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || v.size() > 9 ||
                strtoull(v.c_str(), nullptr, 10) < 2)
                arg_error("Invalid value for '--blocks-min-sites' (at least 2):", v.c_str());
            o.blocks_min_sites = (uint32_t)strtoull(v.c_str(), nullptr, 10);
            o.have_blocks_min = true;
        } else if (a == "--matrix-output") {
            o.matrix_output = need("--matrix-output");
        } else if (a == "--matrix-stat") {
            const std::string k = need("--matrix-stat");
            if (k != "r" && k != "r2" && k != "d" && k != "dprime") arg_error("Invalid value for '--matrix-stat':", k.c_str());
            o.matrix_stat = k == "r" ? WLD_MATRIX_R : k == "r2" ? WLD_MATRIX_R2 : k == "d" ? WLD_MATRIX_D : WLD_MATRIX_DPRIME;
            o.have_matrix_stat = true;
        } else if (a == "--matrix-region") {
            const std::string v = need("--matrix-region");
            const size_t c = v.find(':');
            const std::string lo = v.substr(0, std::min(c, v.size())), hi = c == std::string::npos ? "" : v.substr(c + 1);
            auto bad = [](const std::string &t) {
                return t.empty() || t.find_first_not_of("0123456789") != std::string::npos || t.size() > 19;
            };
            if (bad(lo) || bad(hi) || strtoull(lo.c_str(), nullptr, 10) > strtoull(hi.c_str(), nullptr, 10))
                arg_error("Invalid value for '--matrix-region' (START:END):", v.c_str());
            o.matrix_lo = strtoull(lo.c_str(), nullptr, 10);
            o.matrix_hi = strtoull(hi.c_str(), nullptr, 10);
            o.have_matrix_region = true;
        } else if (a == "--matrix-format") {
            const std::string k = need("--matrix-format");
            if (k != "tsv" && k != "npy") arg_error("Invalid value for '--matrix-format':", k.c_str());
            o.matrix_npy = k == "npy";
            o.have_matrix_format = true;
        } else if (a == "--matrix-zero-missing") {
            o.matrix_zero_missing = true;
        } else if (a == "--matrix-banded") {
            o.matrix_banded = true;
        } else if (a == "--omega-output") {
            o.omega_output = need("--omega-output");
        } else if (a == "--omega-max-side" || a == "--omega-grid" || a == "--omega-min-side" || a == "--omega-max-distance") {
            const std::string name = a;
            const std::string v = need(name.c_str());
            const bool wide = name == "--omega-max-distance";
            if (v.empty() || v.find_first_not_of("0123456789") != std::string::npos || v.size() > (wide ? 19u : 9u))
                arg_error(("Invalid value for '" + name + "':").c_str(), v.c_str());
            const uint64_t x = strtoull(v.c_str(), nullptr, 10);
            if ((name == "--omega-max-side" && x < 1) || (name == "--omega-min-side" && x < 2))
                arg_error(("Invalid value for '" + name + "' (too small):").c_str(), v.c_str());
            if (o.omega_opt.empty()) o.omega_opt = name;
            if (name == "--omega-max-side") o.omega_max_side = (uint32_t)x, o.have_omega_max_side = true;
            else if (name == "--omega-grid") o.omega_grid = (uint32_t)x;
            else if (name == "--omega-min-side") o.omega_min_side = (uint32_t)x;
            else o.omega_max_distance = x;
        } else if (a == "--omega-eps") {
            const std::string v = need("--omega-eps");
            char *end = nullptr;
            o.omega_eps = strtod(v.c_str(), &end);
            if (v.empty() || !end || *end || !(o.omega_eps >= 0.0) || o.omega_eps > 1.79769313486231570815e308)
                arg_error("Invalid value for '--omega-eps' (finite, at least 0):", v.c_str());
            if (o.omega_opt.empty()) o.omega_opt = "--omega-eps";
        } else if (a == "--annot-input") {
            o.annot_input = need("--annot-input");
        } else if (a == "--annot-score-output") {
            o.annot_score_output = need("--annot-score-output");
        } else if (a == "--annot-self") {
            o.annot_self = true;
        } else if (a == "--kernel") {
            std::string k = need("--kernel");
            o.kernel = k == "valu" ? WLD_KERNEL_VALU : k == "mfma" ? WLD_KERNEL_MFMA : WLD_KERNEL_AUTO;
            if (k != "valu" && k != "mfma" && k != "auto") arg_error("Invalid value for '--kernel':", k.c_str());
        } else {
            arg_error("Found argument which wasn't expected, or isn't valid in this context:", argv[i]);
        }
    }
    if (o.fasta_input.empty() && o.vcf_input.empty())
        arg_error("The following required arguments were not provided:", "--fasta-input <fasta-input>");
    const bool ld_sel = o.have_ld_sites || !o.ld_sites_file.empty();
    if (ld_sel && o.ld_sites_output.empty())
        arg_error("The following required arguments were not provided:", "--ld-sites-output <ld-sites-output>");
    if (!ld_sel && !o.ld_sites_output.empty())
        arg_error("The argument '--ld-sites-output' needs", "--ld-sites <ld-sites> or --ld-sites-file <ld-sites-file>");
    if (!ld_sel && o.have_ld_sites_r2) arg_error("The argument '--ld-sites-r2' needs", "--ld-sites-output <ld-sites-output>");
    if (ld_sel && o.devices.size() > 1)
        arg_error("The argument '--ld-sites-output' cannot be used with", "--devices (target sites run on one device)");
    if (!o.partners_output.empty() && !o.have_partners_k)
        arg_error("The following required arguments were not provided:", "--partners-k <partners-k>");
    if (o.partners_output.empty() && o.have_partners_k)
        arg_error("The argument '--partners-k' needs", "--partners-output <partners-output>");
    if (o.partners_output.empty() && o.have_partners_r2)
        arg_error("The argument '--partners-r2' needs", "--partners-output <partners-output>");
    if (!o.blocks_output.empty() && !o.have_blocks_r2 && !o.have_blocks_dprime)
        arg_error("The following required arguments were not provided:",
                  "--blocks-r2 <blocks-r2> or --blocks-dprime <blocks-dprime>");
    if (o.have_blocks_r2 && o.have_blocks_dprime)
        arg_error("The argument '--blocks-r2' cannot be used with", "--blocks-dprime");
    if (o.blocks_output.empty() && (o.have_blocks_r2 || o.have_blocks_dprime || o.have_blocks_rule || o.have_blocks_min))
        arg_error(o.have_blocks_r2       ? "The argument '--blocks-r2' needs"
                  : o.have_blocks_dprime ? "The argument '--blocks-dprime' needs"
                  : o.have_blocks_rule   ? "The argument '--blocks-rule' needs"
                                         : "The argument '--blocks-min-sites' needs",
                  "--blocks-output <blocks-output>");
    if (!o.annot_input.empty() && o.annot_score_output.empty())
        arg_error("The argument '--annot-input' needs", "--annot-score-output <annot-score-output>");
    if (o.annot_input.empty() && !o.annot_score_output.empty())
        arg_error("The argument '--annot-score-output' needs", "--annot-input <annot-input>");
    if (o.annot_self && o.annot_score_output.empty())
        arg_error("The argument '--annot-self' needs", "--annot-input <annot-input> and --annot-score-output <annot-score-output>");
    if (o.matrix_output.empty() &&
        (o.have_matrix_stat || o.have_matrix_region || o.have_matrix_format || o.matrix_zero_missing || o.matrix_banded))
        arg_error(o.have_matrix_stat      ? "The argument '--matrix-stat' needs"
                  : o.have_matrix_region  ? "The argument '--matrix-region' needs"
                  : o.have_matrix_format  ? "The argument '--matrix-format' needs"
                  : o.matrix_zero_missing ? "The argument '--matrix-zero-missing' needs"
                                          : "The argument '--matrix-banded' needs",
                  "--matrix-output <matrix-output>");
    if (o.matrix_banded && !o.matrix_npy)
        arg_error("The argument '--matrix-banded' needs", "--matrix-format npy (a band has no tsv form)");
    if (o.matrix_banded && o.have_matrix_region)
        arg_error("The argument '--matrix-banded' cannot be used with", "--matrix-region (the band holds every site of interest)");
    if (o.matrix_banded && !o.max_distance && !o.max_sites)
        arg_error("The argument '--matrix-banded' needs", "--max-distance or --max-sites (without a window the band is the square)");
    if (!o.omega_output.empty() && !o.have_omega_max_side)
        arg_error("The following required arguments were not provided:", "--omega-max-side <omega-max-side>");
    if (o.omega_output.empty() && !o.omega_opt.empty())
        arg_error(("The argument '" + o.omega_opt + "' needs").c_str(), "--omega-output <omega-output>");
    if (!o.omega_output.empty() && o.devices.size() > 1)
        arg_error("The argument '--omega-output' cannot be used with", "--devices (the sweep scan runs on one device)");
    if (!o.matrix_output.empty() && o.devices.size() > 1)
        arg_error("The argument '--matrix-output' cannot be used with", "--devices (the LD matrix runs on one device)");
    if (!have_pair && !ld_sel && o.partners_output.empty() && o.blocks_output.empty() && o.annot_score_output.empty() &&
        o.matrix_output.empty() && o.omega_output.empty())
        arg_error("The following required arguments were not provided:", "--pair-output <pair-output>");
    if (!o.have_ld_sites_r2) o.ld_sites_r2 = o.r2_threshold;
    if (!o.have_partners_r2) o.partners_r2 = o.r2_threshold;
    if (!o.decay_output.empty() && !o.decay_bin_width)
        arg_error("The following required arguments were not provided:", "--decay-bin-width <decay-bin-width>");
    if (o.decay_output.empty() && o.decay_bin_width)
        arg_error("The argument '--decay-bin-width' needs", "--decay-output <decay-output>");
    if (!o.decay_output.empty() && (o.decay_bins < 1 || o.decay_bins > 1024))
        arg_error("Invalid value for '--decay-bins' (1 to 1024):", std::to_string(o.decay_bins).c_str());
    if (!o.heatmap_output.empty() && !o.have_heatmap_width && !o.have_heatmap_sites)
        arg_error("The following required arguments were not provided:",
                  "--heatmap-cell-width <heatmap-cell-width> or --heatmap-cell-sites <heatmap-cell-sites>");
    if (o.have_heatmap_width && o.have_heatmap_sites)
        arg_error("The argument '--heatmap-cell-width' cannot be used with", "--heatmap-cell-sites");
    if (o.heatmap_output.empty() && (o.have_heatmap_width || o.have_heatmap_sites))
        arg_error(o.have_heatmap_width ? "The argument '--heatmap-cell-width' needs" : "The argument '--heatmap-cell-sites' needs",
                  "--heatmap-output <heatmap-output>");
    if (o.heatmap_output.empty() && (o.have_heatmap_region || o.have_heatmap_stat))
        arg_error(o.have_heatmap_region ? "The argument '--heatmap-region' needs" : "The argument '--heatmap-stat' needs",
                  "--heatmap-output <heatmap-output>");
    if (!o.prune_output.empty() && !o.have_prune_r2)
        arg_error("The following required arguments were not provided:", "--prune-r2 <prune-r2>");
    if (o.prune_output.empty() && o.have_prune_r2)
        arg_error("The argument '--prune-r2' needs", "--prune-output <prune-output>");
    if (!o.prune_output.empty() && o.devices.size() > 1)
        arg_error("The argument '--prune-output' cannot be used with", "--devices (pruning runs on one device)");
    if (o.gpu_prepass && o.devices.size() > 1)
        arg_error("The argument '--gpu-prepass' cannot be used with", "--devices (the device pre-pass runs on one device)");
    return o;
}

// Ends the process from any point after the device-context thread started:
// streams are flushed, but no static destructor runs — the HIP runtime may
// still be starting up on that thread, and tearing it down underneath it
// crashes (SIGSEGV seen on the GPU box).  A Rust panic likewise just ends the
// process with the other threads still running.
[[noreturn]] void quit(int code) {
    fflush(nullptr);
    _exit(code);
}

// Rust's `main() -> Result<(), io::Error>` prints "Error: ..." and exits 1;
// a panic prints the panic message and exits 101.
// msg: the failed call's wld_last_error() (thread-local: pass it when the call
// ran on another thread).
[[noreturn]] void die(int st, const char *what, const char *msg = nullptr) {
    if (!msg) msg = wld_last_error();
    if (st == WLD_E_FORMAT || st == WLD_E_ARG) {
        fprintf(stderr, "thread 'main' panicked at '%s: %s'\n", what, msg);
        quit(101);
    }
    fprintf(stderr, "Error: %s: %s (%s)\n", what, wld_status_string(st), msg);
    quit(1);
}

std::string debug_path(const std::string &p) { return "\"" + p + "\""; }

// main.rs:70-80
int write_henikoff_weights(const std::string &path, const std::vector<float> &w) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return WLD_E_IO;
    std::string out = "Sequence_index\thk_weight\n";
    char buf[64];
    for (size_t i = 0; i < w.size(); ++i) {
        int n = fmt_u64(buf, i);
        buf[n++] = '\t';
        n += fmt3(buf + n, w[i]);
        buf[n++] = '\n';
        out.append(buf, n);
    }
    size_t ok = fwrite(out.data(), 1, out.size(), f);
    int rc = fclose(f);
    return (ok == out.size() && rc == 0) ? WLD_OK : WLD_E_IO;
}

// main.rs:82-119: header, then "{}\t{}\t{:.3}\t{:.3}\t{:.3}" per row in PairStore order.
// Worker threads claim blocks of rows in order and format them into a ring of
// slot buffers; the calling thread writes finished blocks in order, so
// formatting overlaps the file write and memory stays at 2 slots per worker.
int write_pair_stats(const std::string &path, const wld_pairs &p) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return WLD_E_IO;
    const char *hdr = "site_a\tsite_b\td\td'\tr2\n";
    bool ok = fwrite(hdr, 1, strlen(hdr), f) == strlen(hdr);
    const uint64_t n = p.n, block = 1 << 16;
    const uint64_t n_blocks = (n + block - 1) / block;
    ProgressBar pb(n);  // main.rs:89-97: set_position every 5000 rows written (main.rs:111-116)
    const unsigned nt =
        (unsigned)std::max<uint64_t>(1, std::min<uint64_t>({std::thread::hardware_concurrency(), 32, n_blocks}));
    const uint64_t n_slots = 2 * (uint64_t)nt;
    struct Slot {
        std::vector<char> buf;
        size_t len = 0;
        uint64_t ready = UINT64_MAX;  // block index whose text the slot holds
    };
    std::vector<Slot> slots(n_slots);
    std::mutex mu;
    std::condition_variable cv_ready, cv_free;
    uint64_t next_claim = 0, next_write = 0;
    bool abort = false;
    auto worker = [&] {
        for (;;) {
            uint64_t b;
            {
                std::unique_lock<std::mutex> lk(mu);
                if (next_claim >= n_blocks || abort) return;
                b = next_claim++;
                // slot b % n_slots is free once block b - n_slots has been written
                cv_free.wait(lk, [&] { return abort || next_write + n_slots > b; });
                if (abort) return;
            }
            Slot &sl = slots[b % n_slots];
            const uint64_t lo = b * block, hi = std::min(n, lo + block);
            if (sl.buf.size() < (hi - lo) * 48) sl.buf.resize((hi - lo) * 48);
            size_t k = 0;
            for (uint64_t i = lo; i < hi; ++i) {
                if (k + 256 > sl.buf.size()) sl.buf.resize(sl.buf.size() * 2);
                char *o = sl.buf.data() + k;
                int m = fmt_u64(o, p.site_a[i]);
                o[m++] = '\t';
                m += fmt_u64(o + m, p.site_b[i]);
                o[m++] = '\t';
                m += fmt3(o + m, p.d[i]);
                o[m++] = '\t';
                m += fmt3(o + m, p.d_prime[i]);
                o[m++] = '\t';
                m += fmt3(o + m, p.r2[i]);
                o[m++] = '\n';
                k += m;
            }
            {
                std::lock_guard<std::mutex> lk(mu);
                sl.len = k;
                sl.ready = b;
            }
            cv_ready.notify_all();
        }
    };
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt && n_blocks; ++t) th.emplace_back(worker);
    for (uint64_t b = 0; b < n_blocks; ++b) {
        Slot &sl = slots[b % n_slots];
        {
            std::unique_lock<std::mutex> lk(mu);
            cv_ready.wait(lk, [&] { return sl.ready == b; });
        }
        if (ok && fwrite(sl.buf.data(), 1, sl.len, f) != sl.len) ok = false;
        const uint64_t written = std::min(n, (b + 1) * block);
        if (written / 5000 > b * block / 5000) pb.set_position(written / 5000 * 5000);
        {
            std::lock_guard<std::mutex> lk(mu);
            sl.ready = UINT64_MAX;
            ++next_write;
            if (!ok) abort = true;
        }
        cv_free.notify_all();
        if (!ok) break;
    }
    for (auto &x : th) x.join();
    if (fclose(f) != 0) ok = false;
    return ok ? WLD_OK : WLD_E_IO;
}

// --ld-score-output / --decay-output: one summary pass over every in-window
// pair of the loaded set (wld_run_summary: same r2 as the pair TSV's rows, no
// threshold), then the two TSVs.  parent[i]: the parent index of loaded site
// i, as in the pair TSV.  Doubles print as %.9g; an empty bin's mean as nan.
void write_summaries(const Opt &opt, wld_ctx *ctx, const std::vector<uint64_t> &parent) {
    if (opt.ld_score_output.empty() && opt.decay_output.empty()) return;
    using clk = std::chrono::steady_clock;
    const auto sw = clk::now();
    const bool decay = !opt.decay_output.empty();
    wld_summary s;
    const int st = wld_run_summary(ctx, 0, 0, decay ? opt.decay_bin_width : 0, decay ? (uint32_t)opt.decay_bins : 0, &s);
    if (st != WLD_OK) die(st, "run_summary");
    INFO("Summarized %s pairs (%s without a statistic) in %s", human((double)s.pairs).c_str(),
         human((double)(s.none_pairs + s.nonfinite_pairs)).c_str(), fmt_duration(clk::now() - sw).c_str());
    auto write = [&](const std::string &path, const std::string &text) {
        INFO("Writing output to %s", debug_path(path).c_str());
        FILE *f = fopen(path.c_str(), "wb");
        const bool ok = f && fwrite(text.data(), 1, text.size(), f) == text.size();
        if ((f && fclose(f) != 0) || !ok) {
            fprintf(stderr, "Error: cannot write %s\n", path.c_str());
            quit(1);
        }
    };
    char line[160];
    if (!opt.ld_score_output.empty()) {
        std::string out = "site\tpartners\tld_score\n";
        for (uint64_t i = 0; i < s.n_sites; ++i) {
            snprintf(line, sizeof line, "%" PRIu64 "\t%u\t%.9g\n", parent[i], s.partners[i], s.score[i]);
            out += line;
        }
        write(opt.ld_score_output, out);
    }
    if (decay) {
        std::string out = "bin_start\tpairs\tr2_sum\tmean_r2\n";
        for (uint32_t k = 0; k < s.n_bins; ++k) {
            const int n = snprintf(line, sizeof line, "%" PRIu64 "\t%" PRIu64 "\t%.9g\t", (uint64_t)k * s.bin_width,
                                   s.bin_pairs[k], s.bin_r2_sum[k]);
            if (s.bin_pairs[k]) snprintf(line + n, sizeof line - n, "%.9g\n", s.bin_r2_sum[k] / (double)s.bin_pairs[k]);
            else snprintf(line + n, sizeof line - n, "nan\n");
            out += line;
        }
        write(opt.decay_output, out);
    }
    wld_summary_free(&s);
}

// --heatmap-output: the site -> cell map of the loaded set (parent[i] as in
// write_summaries) — equal bins of --heatmap-cell-width coordinates from the
// region's start (without a region: from the multiple of the width at or below
// the first site), or equal runs of --heatmap-cell-sites sites — and the
// coordinate every cell begins at.  Sites outside --heatmap-region are on no
// cell.  More than 4,096 cells, or no site on a cell, ends the run before any
// pair is computed.
struct HeatCells {
    std::vector<int32_t> site_cell;
    std::vector<uint64_t> cell_start;
};
HeatCells resolve_heat_cells(const Opt &opt, const std::vector<uint64_t> &parent) {
    HeatCells h;
    if (opt.heatmap_output.empty()) return h;
    h.site_cell.assign(parent.size(), -1);
    auto inside = [&](uint64_t p) { return !opt.have_heatmap_region || (p >= opt.heatmap_lo && p < opt.heatmap_hi); };
    uint64_t n_cells = 0;
    if (opt.have_heatmap_sites) {
        uint64_t k = 0;
        for (size_t i = 0; i < parent.size(); ++i) {
            if (!inside(parent[i])) continue;
            if (k % opt.heatmap_cell_sites == 0 && k / opt.heatmap_cell_sites < WLD_HEAT_MAX_CELLS) h.cell_start.push_back(parent[i]);
            h.site_cell[i] = (int32_t)std::min<uint64_t>(k / opt.heatmap_cell_sites, WLD_HEAT_MAX_CELLS);
            ++k;
        }
        n_cells = (k + opt.heatmap_cell_sites - 1) / opt.heatmap_cell_sites;
    } else {
        bool any = false;
        uint64_t first = 0;
        for (const uint64_t p : parent)
            if (inside(p) && (!any || p < first)) first = p, any = true;
        const uint64_t W = opt.heatmap_cell_width, origin = opt.have_heatmap_region ? opt.heatmap_lo : first / W * W;
        for (size_t i = 0; i < parent.size() && any; ++i) {
            if (!inside(parent[i])) continue;
            const uint64_t c = (parent[i] - origin) / W;
            n_cells = std::max(n_cells, c + 1);
            h.site_cell[i] = (int32_t)std::min<uint64_t>(c, WLD_HEAT_MAX_CELLS);
        }
        for (uint64_t c = 0; c < std::min<uint64_t>(n_cells, WLD_HEAT_MAX_CELLS); ++c) h.cell_start.push_back(origin + c * W);
    }
    if (n_cells > WLD_HEAT_MAX_CELLS) {
        fprintf(stderr, "error: --heatmap-output: %" PRIu64 " cells; a heat map has at most %d per side (use larger cells "
                        "or a --heatmap-region)\n", n_cells, WLD_HEAT_MAX_CELLS);
        quit(1);
    }
    if (n_cells == 0) {
        fprintf(stderr, "error: --heatmap-output: no site of interest is on a cell\n");
        quit(1);
    }
    return h;
}

// --heatmap-output: one heat-map pass over every in-window pair of the cells'
// sites (wld_run_heatmap: the values of the pair TSV's rows, no threshold),
// then the TSV: the cells with a pair in (i, j) order, i <= j.  Numbers print
// as %.9g (the f32 max round-trips).
void write_heatmap(const Opt &opt, wld_ctx *ctx, const HeatCells &cells) {
    if (opt.heatmap_output.empty()) return;
    using clk = std::chrono::steady_clock;
    const auto sw = clk::now();
    const uint32_t n = (uint32_t)cells.cell_start.size();
    wld_heatmap h;
    const int st = wld_run_heatmap(ctx, cells.site_cell.data(), n, opt.heatmap_stat, 0, 0, &h);
    if (st != WLD_OK) die(st, "run_heatmap");
    INFO("Reduced %s pairs (%s without a statistic) over %u x %u cells, %" PRIu64 " tiles, in %s",
         human((double)h.pairs).c_str(), human((double)(h.none_pairs + h.nonfinite_pairs)).c_str(), n, n, h.tiles,
         fmt_duration(clk::now() - sw).c_str());
    INFO("Writing output to %s", debug_path(opt.heatmap_output).c_str());
    std::string out = "cell_a_start\tcell_b_start\tpairs\tsum\tmean\tmax\n";
    char line[200];
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = i; j < n; ++j) {
            const size_t k = (size_t)i * n + j;
            if (!h.count[k]) continue;
            snprintf(line, sizeof line, "%" PRIu64 "\t%" PRIu64 "\t%" PRIu64 "\t%.9g\t%.9g\t%.9g\n", cells.cell_start[i],
                     cells.cell_start[j], h.count[k], h.sum[k], h.sum[k] / (double)h.count[k], (double)h.max[k]);
            out += line;
        }
    FILE *f = fopen(opt.heatmap_output.c_str(), "wb");
    const bool ok = f && fwrite(out.data(), 1, out.size(), f) == out.size();
    if ((f && fclose(f) != 0) || !ok) {
        fprintf(stderr, "Error: cannot write %s\n", opt.heatmap_output.c_str());
        quit(1);
    }
    wld_heatmap_free(&h);
}

// The "maf" priority of a site from its histogram: minor / (major + minor) of
// the counts of wld_major_minor's symbols, in double, as a float; 0 for a site
// without both.
float maf_priority(const wld_siteset *s, size_t site) {
    uint64_t h[6];
    int major = WLD_NONE, minor = WLD_NONE;
    if (wld_siteset_histogram(s, site, h) != WLD_OK || wld_major_minor(h, &major, &minor) != WLD_OK) return 0.0f;
    if (major < 0 || minor < 0) return 0.0f;
    return (float)((double)h[minor] / ((double)h[major] + (double)h[minor]));
}

// --prune-output: the greedy r2-independent site set of the loaded set at
// --prune-r2 under the window (wld_run_prune), one line per loaded site in
// loaded order.  parent[i] as in write_summaries; hist_set/hist_index: where
// loaded site i's histogram is found (--prune-priority maf).
void write_prune(const Opt &opt, wld_ctx *ctx, const std::vector<uint64_t> &parent, const wld_siteset *hist_set,
                 const std::vector<size_t> &hist_index) {
    if (opt.prune_output.empty()) return;
    using clk = std::chrono::steady_clock;
    const auto sw = clk::now();
    std::vector<float> priority;
    if (opt.prune_maf) {
        priority.resize(parent.size());
        for (size_t i = 0; i < parent.size(); ++i) priority[i] = maf_priority(hist_set, hist_index[i]);
    }
    wld_prune p;
    const int st = wld_run_prune(ctx, opt.prune_r2, opt.prune_maf ? priority.data() : nullptr, &p);
    if (st != WLD_OK) die(st, "run_prune");
    INFO("Pruned %" PRIu64 " sites to %" PRIu64 " (%s pairs above r2 %g) in %s", p.n_sites, p.n_kept,
         human((double)p.edges).c_str(), (double)opt.prune_r2, fmt_duration(clk::now() - sw).c_str());
    INFO("Writing output to %s", debug_path(opt.prune_output).c_str());
    std::string out = "site\tkept\ttag\n";
    char line[96];
    for (uint64_t i = 0; i < p.n_sites; ++i) {
        snprintf(line, sizeof line, "%" PRIu64 "\t%u\t%" PRIu64 "\n", parent[i], (unsigned)p.keep[i], parent[p.tag[i]]);
        out += line;
    }
    FILE *f = fopen(opt.prune_output.c_str(), "wb");
    const bool ok = f && fwrite(out.data(), 1, out.size(), f) == out.size();
    if ((f && fclose(f) != 0) || !ok) {
        fprintf(stderr, "Error: cannot write %s\n", opt.prune_output.c_str());
        quit(1);
    }
    wld_prune_free(&p);
}

// --ld-sites / --ld-sites-file: the target coordinates (the list's, then the
// file's lines) as loaded indices — every loaded site carrying a coordinate,
// in loaded order.  parent[i] as in write_summaries.  A coordinate no loaded
// site carries ends the run, before any pair is computed.
std::vector<uint32_t> resolve_targets(const Opt &opt, const std::vector<uint64_t> &parent) {
    std::vector<uint32_t> t;
    if (opt.ld_sites_output.empty()) return t;
    std::vector<uint64_t> want = opt.ld_sites;
    if (!opt.ld_sites_file.empty()) {
        FILE *f = fopen(opt.ld_sites_file.c_str(), "rb");
        if (!f) {
            fprintf(stderr, "Error: cannot read %s\n", opt.ld_sites_file.c_str());
            quit(1);
        }
        char line[256];
        while (fgets(line, sizeof line, f)) {
            std::string v(line);
            while (!v.empty() && (v.back() == '\n' || v.back() == '\r' || v.back() == ' ' || v.back() == '\t')) v.pop_back();
            if (v.empty()) continue;
            if (v.find_first_not_of("0123456789") != std::string::npos || v.size() > 19) {
                fprintf(stderr, "error: --ld-sites-file %s: '%s' is not a coordinate\n", opt.ld_sites_file.c_str(), v.c_str());
                quit(1);
            }
            want.push_back(strtoull(v.c_str(), nullptr, 10));
        }
        fclose(f);
    }
    for (const uint64_t p : want) {
        const size_t before = t.size();
        for (size_t i = 0; i < parent.size(); ++i)
            if (parent[i] == p) t.push_back((uint32_t)i);
        if (t.size() == before) {
            fprintf(stderr, "error: --ld-sites: no site of interest has coordinate %" PRIu64 "\n", p);
            quit(1);
        }
    }
    return t;
}

// --ld-sites-output: the targets' rows at --ld-sites-r2 under the window
// (wld_run_targets), by target then partner; parent indices and the three
// numbers formatted as the pair TSV's.
void write_targets(const Opt &opt, wld_ctx *ctx, const std::vector<uint32_t> &targets) {
    if (opt.ld_sites_output.empty()) return;
    using clk = std::chrono::steady_clock;
    const auto sw = clk::now();
    wld_target_rows r;
    const int st = wld_run_targets(ctx, targets.data(), (uint32_t)targets.size(), opt.ld_sites_r2, &r);
    if (st != WLD_OK) die(st, "run_targets");
    INFO("Computed %zu target sites: %s rows above r2 %g in %s", targets.size(), human((double)r.n).c_str(),
         (double)opt.ld_sites_r2, fmt_duration(clk::now() - sw).c_str());
    INFO("Writing output to %s", debug_path(opt.ld_sites_output).c_str());
    std::string out = "target\tsite\td\td'\tr2\n";
    char line[160];
    for (uint64_t i = 0; i < r.n; ++i) {
        int m = fmt_u64(line, r.site_target[i]);
        line[m++] = '\t';
        m += fmt_u64(line + m, r.site_partner[i]);
        line[m++] = '\t';
        m += fmt3(line + m, r.d[i]);
        line[m++] = '\t';
        m += fmt3(line + m, r.d_prime[i]);
        line[m++] = '\t';
        m += fmt3(line + m, r.r2[i]);
        line[m++] = '\n';
        out.append(line, m);
    }
    FILE *f = fopen(opt.ld_sites_output.c_str(), "wb");
    const bool ok = f && fwrite(out.data(), 1, out.size(), f) == out.size();
    if ((f && fclose(f) != 0) || !ok) {
        fprintf(stderr, "Error: cannot write %s\n", opt.ld_sites_output.c_str());
        quit(1);
    }
    wld_target_rows_free(&r);
}

// --partners-output: every site's best --partners-k partners at --partners-r2
// under the window (wld_run_partners), by site then rank; parent indices and
// the three numbers formatted as the targets' rows.
void write_partners(const Opt &opt, wld_ctx *ctx, const std::vector<uint64_t> &parent) {
    if (opt.partners_output.empty()) return;
    using clk = std::chrono::steady_clock;
    const auto sw = clk::now();
    wld_partners r;
    const int st = wld_run_partners(ctx, opt.partners_k, opt.partners_r2, 0, 0, &r);
    if (st != WLD_OK) die(st, "run_partners");
    INFO("Computed the best %u partners of %" PRIu64 " sites: %s pairs above r2 %g in %s", opt.partners_k, r.n_sites,
         human((double)r.passing_pairs).c_str(), (double)opt.partners_r2, fmt_duration(clk::now() - sw).c_str());
    INFO("Writing output to %s", debug_path(opt.partners_output).c_str());
    std::string out = "site\tpartner\trank\td\td'\tr2\n";
    char line[200];
    for (uint64_t s = 0; s < r.n_sites && s < parent.size(); ++s)
        for (uint32_t k = 0; k < r.count[s]; ++k) {
            const uint64_t i = s * r.k + k;
            if (r.partner[i] >= parent.size()) continue;
            int m = fmt_u64(line, parent[s]);
            line[m++] = '\t';
            m += fmt_u64(line + m, parent[r.partner[i]]);
            line[m++] = '\t';
            m += fmt_u64(line + m, k);
            line[m++] = '\t';
            m += fmt3(line + m, r.d[i]);
            line[m++] = '\t';
            m += fmt3(line + m, r.d_prime[i]);
            line[m++] = '\t';
            m += fmt3(line + m, r.r2[i]);
            line[m++] = '\n';
            out.append(line, m);
        }
    FILE *f = fopen(opt.partners_output.c_str(), "wb");
    const bool ok = f && fwrite(out.data(), 1, out.size(), f) == out.size();
    if ((f && fclose(f) != 0) || !ok) {
        fprintf(stderr, "Error: cannot write %s\n", opt.partners_output.c_str());
        quit(1);
    }
    wld_partners_free(&r);
}

// --blocks-output: the LD blocks of the loaded set under the window
// (wld_run_blocks), one line per block in site order; first and last are
// parent indices as --prune-output prints sites, mean (rounded to f32) and min
// formatted as the pair TSV's numbers, nan without an informative pair.
void write_blocks(const Opt &opt, wld_ctx *ctx, const std::vector<uint64_t> &parent) {
    if (opt.blocks_output.empty()) return;
    using clk = std::chrono::steady_clock;
    const auto sw = clk::now();
    wld_blocks r;
    const int st = wld_run_blocks(ctx, opt.have_blocks_dprime ? WLD_BLOCKS_ABS_DPRIME : WLD_BLOCKS_R2,
                                  opt.blocks_min_value, opt.blocks_rule, opt.blocks_min_sites, &r);
    if (st != WLD_OK) die(st, "run_blocks");
    INFO("Found %u LD blocks in %" PRIu64 " sites (%s weak of %s pairs at %s %g) in %s", r.n_blocks, r.n_sites,
         human((double)r.break_weak_pairs).c_str(), human((double)r.break_pairs).c_str(),
         opt.have_blocks_dprime ? "|d'|" : "r2", (double)opt.blocks_min_value, fmt_duration(clk::now() - sw).c_str());
    INFO("Writing output to %s", debug_path(opt.blocks_output).c_str());
    std::string out = "block\tfirst\tlast\tsites\tpairs\tinformative\tstrong\tmean\tmin\n";
    char line[256];
    for (uint32_t k = 0; k < r.n_blocks; ++k) {
        if (r.first[k] >= parent.size() || r.last[k] >= parent.size()) continue;
        const uint64_t cols[7] = {k, parent[r.first[k]], parent[r.last[k]], (uint64_t)r.last[k] - r.first[k] + 1,
                                  r.pairs[k], r.informative[k], r.strong[k]};
        int m = 0;
        for (const uint64_t c : cols) {
            m += fmt_u64(line + m, c);
            line[m++] = '\t';
        }
        m += fmt3(line + m, r.informative[k] ? (float)(r.value_sum[k] / (double)r.informative[k]) : std::nanf(""));
        line[m++] = '\t';
        m += fmt3(line + m, r.value_min[k]);
        line[m++] = '\n';
        out.append(line, m);
    }
    FILE *f = fopen(opt.blocks_output.c_str(), "wb");
    const bool ok = f && fwrite(out.data(), 1, out.size(), f) == out.size();
    if ((f && fclose(f) != 0) || !ok) {
        fprintf(stderr, "Error: cannot write %s\n", opt.blocks_output.c_str());
        quit(1);
    }
    wld_blocks_free(&r);
}

// (debug level only, so info-level output is the reference's: the LD pass's
// progress_report calls — progress(0), then one per 256x256 chunk)
void log_progress(const ProgressBar &pb) {
    log_at(4, "progress: %" PRIu64 " progress_report calls, last %" PRIu64 " pairs", pb.updates(),
           pb.last_position());
}

// --annot-input: the file, read and checked right after the arguments (before
// the input set is read and before any device step); a format error ends the
// run with the line it is on.
annot_plan::File read_annot_input(const Opt &opt) {
    annot_plan::File f;
    if (opt.annot_input.empty()) return f;
    std::string err;
    if (!annot_plan::read_file(opt.annot_input.c_str(), f, err)) {
        fprintf(stderr, "error: --annot-input %s: %s\n", opt.annot_input.c_str(), err.c_str());
        exit(1);
    }
    return f;
}

// ... joined to the loaded set (parent[i] as in write_summaries): loaded site i
// takes the first unused row at or after the previous match that carries its
// parent index.  A site of interest without a row ends the run, before any
// pair is computed.
std::vector<float> resolve_annot(const Opt &opt, const annot_plan::File &file, const std::vector<uint64_t> &parent) {
    std::vector<float> annot;
    if (opt.annot_score_output.empty()) return annot;
    std::string err;
    if (!annot_plan::join(file, parent.data(), parent.size(), annot, err)) {
        fprintf(stderr, "error: --annot-input %s: %s\n", opt.annot_input.c_str(), err.c_str());
        quit(1);
    }
    return annot;
}

// --annot-score-output: one pass over every in-window pair of the loaded set
// (wld_run_annot_scores: the r2 of the pair TSV's rows, no threshold), then the
// TSV, one line per loaded site.  Doubles print as %.9g.
void write_annot_scores(const Opt &opt, wld_ctx *ctx, const annot_plan::File &file, const std::vector<float> &annot,
                        const std::vector<uint64_t> &parent) {
    if (opt.annot_score_output.empty()) return;
    using clk = std::chrono::steady_clock;
    const auto sw = clk::now();
    const uint32_t C = (uint32_t)file.names.size();
    wld_annot_scores s;
    const int st = wld_run_annot_scores(ctx, annot.data(), C, opt.annot_self ? WLD_ANNOT_SELF : 0, 0, 0, &s);
    if (st != WLD_OK) die(st, "run_annot_scores");
    INFO("Partitioned the LD scores of %s pairs (%s without a statistic) over %u annotations in %s",
         human((double)s.pairs).c_str(), human((double)(s.none_pairs + s.nonfinite_pairs)).c_str(), C,
         fmt_duration(clk::now() - sw).c_str());
    INFO("Writing output to %s", debug_path(opt.annot_score_output).c_str());
    std::string out = "site\tpartners";
    for (const std::string &n : file.names) out += "\t" + n + "_l2";
    out += "\n";
    char cell[64];
    for (uint64_t i = 0; i < s.n_sites && i < parent.size(); ++i) {
        snprintf(cell, sizeof cell, "%" PRIu64 "\t%u", parent[i], s.partners[i]);
        out += cell;
        for (uint32_t k = 0; k < C; ++k) {
            snprintf(cell, sizeof cell, "\t%.9g", s.score[i * C + k]);
            out += cell;
        }
        out += "\n";
    }
    FILE *f = fopen(opt.annot_score_output.c_str(), "wb");
    const bool ok = f && fwrite(out.data(), 1, out.size(), f) == out.size();
    if ((f && fclose(f) != 0) || !ok) {
        fprintf(stderr, "Error: cannot write %s\n", opt.annot_score_output.c_str());
        quit(1);
    }
    wld_annot_scores_free(&s);
}

// --matrix-output: the loaded-site range of --matrix-region (parent[i] as in
// write_summaries; START <= parent < END, --heatmap-region's rule), one matrix
// call to the host (wld_run_matrix: the values of the pair TSV's rows, no
// threshold), then the TSV (%.9g: an f32 round-trips) or the npy file with the
// parent indices beside it.
void write_matrix(const Opt &opt, wld_ctx *ctx, const std::vector<uint64_t> &parent) {
    if (opt.matrix_output.empty()) return;
    using clk = std::chrono::steady_clock;
    const auto sw = clk::now();
    size_t b = 0, e = parent.size();
    if (opt.have_matrix_region) {
        if (!std::is_sorted(parent.begin(), parent.end())) {
            fprintf(stderr, "error: --matrix-region needs sites in ascending parent order\n");
            quit(1);
        }
        b = std::lower_bound(parent.begin(), parent.end(), opt.matrix_lo) - parent.begin();
        e = std::lower_bound(parent.begin(), parent.end(), opt.matrix_hi) - parent.begin();
    }
    if (e <= b) {
        fprintf(stderr, "error: --matrix-output: no site of interest lies in the region\n");
        quit(1);
    }
    const size_t n = e - b;
    size_t width = n;  // the file's columns: n, or --matrix-banded's K + 1
    std::vector<float> m;
    if (opt.matrix_banded) {
        uint32_t K = 0;
        int st = wld_matrix_banded_width(ctx, &K);
        if (st != WLD_OK) die(st, "matrix_banded_width");
        width = (size_t)K + 1;
        try {
            m.resize(n * width);
        } catch (const std::bad_alloc &) {
            fprintf(stderr, "error: --matrix-output: a %zu x %zu band does not fit in memory\n", n, width);
            quit(1);
        }
        wld_matrix_banded_info info;
        st = wld_run_matrix_banded(ctx, 0, 0, K, opt.matrix_stat, WLD_MATRIX_F32,
                                   opt.matrix_zero_missing ? WLD_MATRIX_ZERO_MISSING : 0, m.data(), width, &info);
        if (st != WLD_OK) die(st, "run_matrix_banded");
        INFO("Computed the %zu x %zu band of the LD matrix from %s pairs (%s without a statistic) in %s", n, width,
             human((double)info.pairs).c_str(), human((double)(info.none_pairs + info.nonfinite_pairs)).c_str(),
             fmt_duration(clk::now() - sw).c_str());
    } else {
        try {
            m.resize(n * n);
        } catch (const std::bad_alloc &) {
            fprintf(stderr, "error: --matrix-output: a %zu x %zu matrix does not fit in memory (use --matrix-region)\n", n, n);
            quit(1);
        }
        wld_matrix_info info;
        const int st = wld_run_matrix(ctx, (uint32_t)b, (uint32_t)e, (uint32_t)b, (uint32_t)e, opt.matrix_stat,
                                      WLD_MATRIX_F32, opt.matrix_zero_missing ? WLD_MATRIX_ZERO_MISSING : 0, m.data(), n,
                                      &info);
        if (st != WLD_OK) die(st, "run_matrix");
        INFO("Computed the %zu x %zu LD matrix from %s pairs (%s without a statistic) in %s", n, n,
             human((double)info.pairs).c_str(), human((double)(info.none_pairs + info.nonfinite_pairs)).c_str(),
             fmt_duration(clk::now() - sw).c_str());
    }
    INFO("Writing output to %s", debug_path(opt.matrix_output).c_str());
    auto write_all = [&](const std::string &path, const std::string &head, const void *body, size_t bytes) {
        FILE *f = fopen(path.c_str(), "wb");
        const bool ok = f && fwrite(head.data(), 1, head.size(), f) == head.size() &&
                        (!bytes || fwrite(body, 1, bytes, f) == bytes);
        if ((f && fclose(f) != 0) || !ok) {
            fprintf(stderr, "Error: cannot write %s\n", path.c_str());
            quit(1);
        }
    };
    char cell[64];
    if (opt.matrix_npy) {
        // npy 1.0: magic, version, u16 header length, a dict padded with spaces
        // to a multiple of 64 bytes in all, newline-terminated
        std::string dict = "{'descr': '<f4', 'fortran_order': False, 'shape': (" + std::to_string(n) + ", " +
                           std::to_string(width) + "), }";
        while ((10 + dict.size() + 1) % 64) dict += ' ';
        dict += '\n';
        std::string head("\x93NUMPY\x01\x00", 8);
        head += (char)(dict.size() & 0xFF);
        head += (char)(dict.size() >> 8);
        head += dict;
        write_all(opt.matrix_output, head, m.data(), m.size() * sizeof(float));
        std::string sites;
        for (size_t i = b; i < e; ++i) {
            snprintf(cell, sizeof cell, "%" PRIu64 "\n", parent[i]);
            sites += cell;
        }
        write_all(opt.matrix_output + ".sites", sites, nullptr, 0);
        return;
    }
    std::string out = "site";
    for (size_t i = b; i < e; ++i) {
        snprintf(cell, sizeof cell, "\t%" PRIu64, parent[i]);
        out += cell;
    }
    out += "\n";
    for (size_t i = 0; i < n; ++i) {
        snprintf(cell, sizeof cell, "%" PRIu64, parent[b + i]);
        out += cell;
        for (size_t j = 0; j < n; ++j) {
            const float x = m[i * n + j];
            if (x != x) snprintf(cell, sizeof cell, "\tnan");
            else snprintf(cell, sizeof cell, "\t%.9g", (double)x);
            out += cell;
        }
        out += "\n";
    }
    write_all(opt.matrix_output, out, nullptr, 0);
}

// --omega-output: the sweep scan of the loaded set (wld_run_omega), one line per
// position: the position and the best borders in parent coordinates (NA where
// no candidate had a positive cross term), omega and zns with 17 significant
// digits, which round-trip the f64 bits.  Without --max-sites the window is set
// to the 2 * max-side - 1 sites the scan needs for this call and put back.
void write_omega(const Opt &opt, wld_ctx *ctx, const std::vector<uint64_t> &parent) {
    if (opt.omega_output.empty()) return;
    using clk = std::chrono::steady_clock;
    const auto sw = clk::now();
    uint64_t win_d = 0, win_k = 0;
    int st = wld_get_window(ctx, &win_d, &win_k);
    if (st != WLD_OK) die(st, "get_window");
    if (!opt.max_sites && (st = wld_set_window(ctx, win_d, 2ull * opt.omega_max_side - 1)) != WLD_OK) die(st, "set_window");
    wld_omega r;
    st = wld_run_omega(ctx, opt.omega_grid, opt.omega_max_side, opt.omega_min_side, opt.omega_max_distance, opt.omega_eps,
                       WLD_MATRIX_F32, &r);
    if (st != WLD_OK) die(st, "run_omega");
    if (!opt.max_sites && (st = wld_set_window(ctx, win_d, win_k)) != WLD_OK) die(st, "set_window");
    INFO("Scanned %u positions for sweeps: %s border pairs evaluated, %s skipped, in %s", r.n_splits,
         human((double)r.scan.evaluated).c_str(), human((double)r.scan.skipped).c_str(),
         fmt_duration(clk::now() - sw).c_str());
    INFO("Writing output to %s", debug_path(opt.omega_output).c_str());
    std::string out = "position\tleft\tright\tomega\tzns\n";
    char line[200];
    for (uint32_t g = 0; g < r.n_splits; ++g) {
        const bool none = r.left[g] == 0xFFFFFFFFu && r.right[g] == 0xFFFFFFFFu;  // (the library's "no candidate")
        if (!none && (r.left[g] >= parent.size() || r.right[g] >= parent.size())) {
            fprintf(stderr, "error: internal: split %u has the borders %u, %u of %zu sites\n", g, r.left[g], r.right[g],
                    parent.size());
            quit(1);
        }
        int m;
        if (none) m = snprintf(line, sizeof line, "%" PRIu64 "\tNA\tNA\tnan\t%.17g\n", r.position[g], r.zns[g]);
        else
            m = snprintf(line, sizeof line, "%" PRIu64 "\t%" PRIu64 "\t%" PRIu64 "\t%.17g\t%.17g\n", r.position[g],
                         parent[r.left[g]], parent[r.right[g]], r.omega[g], r.zns[g]);
        out.append(line, (size_t)m);
    }
    FILE *f = fopen(opt.omega_output.c_str(), "wb");
    const bool ok = f && fwrite(out.data(), 1, out.size(), f) == out.size();
    if ((f && fclose(f) != 0) || !ok) {
        fprintf(stderr, "Error: cannot write %s\n", opt.omega_output.c_str());
        quit(1);
    }
    wld_omega_free(&r);
}

// main.rs:186-212 after the pair computation: timing logs, TSV, clean-up.
int finish(const Opt &opt, wld_ctx *ctx, wld_pairs &pairs, std::chrono::steady_clock::duration dur,
           uint64_t total_pairs) {
    using clk = std::chrono::steady_clock;
    if (opt.pair_output.empty()) {  // (--ld-sites-output alone: no pair pass ran)
        wld_destroy(ctx);
        return 0;
    }
    INFO("Finished computing pairwise weighted LD stats in %s", fmt_duration(dur).c_str());
    const double secs = std::chrono::duration<double>(dur).count();
    INFO("    %s pairs computed at ~%s, %s passed threshold", human((double)total_pairs).c_str(),
         human((double)total_pairs / secs, "pairs/s").c_str(), human((double)pairs.n).c_str());
    wld_run_stats rs;
    if (wld_last_stats(ctx, &rs) == WLD_OK)
        log_at(4, "device: kernel=%s pairs=%" PRIu64 " pair_kernel=%.3fms order=%.3fms",
               rs.kernel == WLD_KERNEL_MFMA ? "mfma" : "valu", rs.pairs, rs.pair_kernel_ms, rs.order_ms);

    INFO("Writing output to %s", debug_path(opt.pair_output).c_str());
    auto sw = clk::now();
    if (write_pair_stats(opt.pair_output, pairs) != WLD_OK) {
        fprintf(stderr, "Error: cannot write %s\n", opt.pair_output.c_str());
        return 1;
    }
    INFO("Finshed writing output in %s", fmt_duration(clk::now() - sw).c_str());  // (sic) main.rs:210
    wld_pairs_free(&pairs);
    wld_destroy(ctx);
    return 0;
}

// --gpu-prepass: main.rs:139-190 with the site filter and Henikoff weights on
// the device (wld_load_filtered), then the staged run and a host copy of the rows.
int run_gpu_prepass(const Opt &opt, wld_siteset *siteset, wld_ctx *ctx, const annot_plan::File &annot_file) {
    using clk = std::chrono::steady_clock;
    const size_t L0 = wld_siteset_n_sites(siteset), N = wld_siteset_n_seqs(siteset);
    auto sw = clk::now();
    size_t L = 0;
    int st = wld_load_filtered(ctx, wld_siteset_buffer(siteset), L0, N, wld_siteset_site_map(siteset), opt.min_acgt,
                               opt.min_minor, opt.max_minor, opt.unweighted ? 1 : 0, &L);
    if (st != WLD_OK) die(st, "load_filtered");
    INFO("Computed + filtered sites of interest%s on the GPU in %s", opt.unweighted ? "" : " and Henikoff weights",
         fmt_duration(clk::now() - sw).c_str());
    INFO("    Found %zu sites of interest", L);
    if (!opt.weights_output.empty()) {
        std::vector<float> weights(N);
        if ((st = wld_weights_copy(ctx, weights.data())) != WLD_OK) die(st, "weights_copy");
        INFO("Writing weights to %s", debug_path(opt.weights_output).c_str());
        if (write_henikoff_weights(opt.weights_output, weights) != WLD_OK) {
            fprintf(stderr, "Error: cannot write %s\n", opt.weights_output.c_str());
            quit(1);  // the context thread may still be running
        }
    }
    std::vector<uint64_t> parent(L);
    if (L && (st = wld_site_map_copy(ctx, parent.data())) != WLD_OK) die(st, "site_map_copy");
    const std::vector<uint32_t> targets = resolve_targets(opt, parent);
    const HeatCells heat_cells = resolve_heat_cells(opt, parent);
    const std::vector<float> annot = resolve_annot(opt, annot_file, parent);
    if (!opt.pair_output.empty()) INFO("Beginning pairwise weighted LD computation");
    sw = clk::now();
    const uint64_t total_pairs = ((uint64_t)L - 1) * ((uint64_t)L - 2) / 2;  // main.rs:168 (sic, wraps)
    wld_pairs pairs{};  // any L: batches of <= 2^31 pairs, rows appended in reference order
    if (!opt.pair_output.empty()) {
        ProgressBar pb(total_pairs);  // main.rs:170-178
        on_progress(0, &pb);  // all_weighted_ld_pairs' initial report (lib.rs:584); wld_run_host reports chunks only
        if ((st = wld_run_host(ctx, opt.r2_threshold, on_progress, &pb, &pairs)) != WLD_OK)
            die(st, "all_weighted_ld_pairs");
        log_progress(pb);
    }
    const auto dur = clk::now() - sw;
    write_summaries(opt, ctx, parent);
    write_heatmap(opt, ctx, heat_cells);
    write_targets(opt, ctx, targets);
    write_partners(opt, ctx, parent);
    write_blocks(opt, ctx, parent);
    write_annot_scores(opt, ctx, annot_file, annot, parent);
    write_matrix(opt, ctx, parent);
    write_omega(opt, ctx, parent);
    // (a FASTA set has no site_map: a kept site's parent index is its index in the unfiltered set)
    write_prune(opt, ctx, parent, siteset, std::vector<size_t>(parent.begin(), parent.end()));
    return finish(opt, ctx, pairs, dur, total_pairs);
}

}  // namespace

int main(int argc, char **argv) {
    init_logger();
    Opt opt = parse(argc, argv);
    const annot_plan::File annot_file = read_annot_input(opt);
    using clk = std::chrono::steady_clock;
    if (opt.exact_sums) {
        // not a reference flag (main.rs:14-68 has none like it): printed at any
        // log level, since the TSV it produces is not lib.rs's
        const int keep = g_level;
        g_level = std::max(g_level, 2);
        log_at(2, "--exact-sums departs from the reference: the masked sums are exact sums rounded once, not "
                  "lib.rs's f32 summation order, so d, d' and r2 differ from lib.rs's where its own f32 rounding "
                  "shows (measured on rare-allele data: |d'| up to 1.11, |r2| up to 0.023 against lib.rs); "
                  "without the flag the output is lib.rs's, bit for bit");
        g_level = keep;
    }

    // The device context (HIP runtime start-up) is created while the input is
    // read, so that the LD timing below covers the computation only.
    wld_ctx *ctx = nullptr;
    int ctx_st = WLD_OK;
    std::string ctx_msg;
    std::thread ctx_thread([&] {
        ctx_st = opt.devices.empty() ? wld_create(opt.device, &ctx)
                                     : wld_create_multi(opt.devices.data(), (int)opt.devices.size(), &ctx);
        if (ctx_st != WLD_OK) ctx_msg = wld_last_error();
    });
    auto get_ctx = [&]() -> wld_ctx * {
        if (ctx_thread.joinable()) ctx_thread.join();
        if (ctx_st != WLD_OK) die(ctx_st, "wld_create", ctx_msg.c_str());
        if (opt.kernel != WLD_KERNEL_AUTO) {
            int s2 = wld_set_kernel(ctx, opt.kernel);
            if (s2 != WLD_OK) die(s2, "wld_set_kernel");
        }
        if (opt.exact_sums) {
            int s2 = wld_set_option(ctx, WLD_OPT_REF_SUMS, 0);
            if (s2 != WLD_OK) die(s2, "wld_set_option");
        }
        if (opt.max_distance || opt.max_sites) {
            int s2 = wld_set_window(ctx, opt.max_distance, opt.max_sites);
            if (s2 != WLD_OK) die(s2, "wld_set_window");
        }
        return ctx;
    };

    auto sw = clk::now();
    wld_siteset *siteset = nullptr;
    int st;
    const bool vcf = !opt.vcf_input.empty();
    if (vcf)
        st = wld_read_vcf(opt.vcf_input.c_str(), &siteset);
    else
        st = wld_read_fasta(opt.fasta_input.c_str(), &siteset);
    if (st != WLD_OK) die(st, vcf ? "read_vcf" : "read_fasta");
    INFO("Loaded %s file in %s", vcf ? "vcf" : "fasta", fmt_duration(clk::now() - sw).c_str());
    INFO("    %zu sequences, %zu sites", wld_siteset_n_seqs(siteset), wld_siteset_n_sites(siteset));

    if (opt.gpu_prepass && !vcf) return run_gpu_prepass(opt, siteset, get_ctx(), annot_file);

    sw = clk::now();
    wld_siteset *filtered = nullptr;
    if (vcf) {
        // handle_vcf has no variable-site filter (WeightedLD.py:382-402)
        filtered = siteset;
        siteset = nullptr;
        INFO("VCF input: no site filter (WeightedLD.py handle_vcf semantics)");
    } else {
        st = wld_siteset_filter_sites_of_interest(siteset, opt.min_acgt, opt.min_minor, opt.max_minor, &filtered);
        if (st != WLD_OK) die(st, "filter_by");
        INFO("Computed + filtered sites of interest in %s", fmt_duration(clk::now() - sw).c_str());
    }
    const size_t L = wld_siteset_n_sites(filtered), N = wld_siteset_n_seqs(filtered);
    INFO("    Found %zu sites of interest", L);

    std::vector<float> weights(N, 1.0f);
    if (!opt.unweighted) {
        sw = clk::now();
        st = wld_henikoff_weights(filtered, weights.data());
        if (st != WLD_OK) die(st, "henikoff_weights");
        INFO("Computed Henikoff weights in %s", fmt_duration(clk::now() - sw).c_str());
    }
    if (!opt.weights_output.empty()) {
        INFO("Writing weights to %s", debug_path(opt.weights_output).c_str());
        if (write_henikoff_weights(opt.weights_output, weights) != WLD_OK) {
            fprintf(stderr, "Error: cannot write %s\n", opt.weights_output.c_str());
            quit(1);  // the context thread may still be running
        }
    }

    std::vector<uint64_t> parent(L);
    for (size_t i = 0; i < L; ++i) parent[i] = wld_siteset_parent_site_index(filtered, i);
    const std::vector<uint32_t> targets = resolve_targets(opt, parent);
    const HeatCells heat_cells = resolve_heat_cells(opt, parent);
    const std::vector<float> annot = resolve_annot(opt, annot_file, parent);
    if (!opt.pair_output.empty()) INFO("Beginning pairwise weighted LD computation");
    sw = clk::now();
    const uint64_t total_pairs = ((uint64_t)L - 1) * ((uint64_t)L - 2) / 2;  // main.rs:168 (sic, wraps)
    get_ctx();
    wld_pairs pairs{};
    if (opt.pair_output.empty()) {  // (--ld-sites-output alone: the load, no pair pass)
        st = wld_load(ctx, wld_siteset_buffer(filtered), L, N, wld_siteset_site_map(filtered), weights.data());
        if (st != WLD_OK) die(st, "load");
    } else {
        ProgressBar pb(total_pairs);  // main.rs:170-178, fed by the closure of main.rs:184-188
        st = wld_all_weighted_ld_pairs(ctx, wld_siteset_buffer(filtered), L, N, wld_siteset_site_map(filtered),
                                       weights.data(), opt.r2_threshold, on_progress, &pb, &pairs);
        if (st != WLD_OK) die(st, "all_weighted_ld_pairs");
        log_progress(pb);
    }
    const auto dur = clk::now() - sw;
    write_summaries(opt, ctx, parent);
    write_heatmap(opt, ctx, heat_cells);
    write_targets(opt, ctx, targets);
    write_partners(opt, ctx, parent);
    write_blocks(opt, ctx, parent);
    write_annot_scores(opt, ctx, annot_file, annot, parent);
    write_matrix(opt, ctx, parent);
    write_omega(opt, ctx, parent);
    std::vector<size_t> self(L);
    for (size_t i = 0; i < L; ++i) self[i] = i;
    write_prune(opt, ctx, parent, filtered, self);
    const int rc = finish(opt, ctx, pairs, dur, total_pairs);
    wld_siteset_free(filtered);
    wld_siteset_free(siteset);
    return rc;
}
