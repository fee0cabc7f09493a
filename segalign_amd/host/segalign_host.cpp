// segalign_host.cpp -- host harness for the MI355X engine: FASTA in, LASTZ ".segments" files + lastz command lines out.
//
// SURVEY.md 8(f) rows 2 and 3.  The reference host (src/main.cpp + src/seeder.cpp + src/segment_printer.cpp) needs
// TBB, boost and kentUtils and "stays intact" upstream; this program is the small owned driver that walks the same
// engine boundary in the same order so that the whole path can be run and measured end to end without them:
//
//   sequence arenas     src/main.cpp:300-549   records joined by '&', blocks closed once they exceed seq_block_size,
//                                              reverse-complement arena per query block, *_block<k>.name files
//   work plan           src/main.cpp:383-393   10 Mbp intervals per query block ; src/seeder.cpp:48-51 250 kbp chunks
//   engine call order   src/main.cpp:297-298,613-621,649-685,743 (InitializeInterface, InitializeProcessor, per target
//                       block: ClearRef/SendRef/GenerateSeedPosTable, query blocks through BUFFER_DEPTH=2 device buffers)
//   seeder body         src/seeder.cpp:12-127  per interval: plus strand chunks, then minus strand chunks in rc coordinates
//   segment printer     src/segment_printer.cpp:11-173  tmp<i>.block<q>.r<rstart>.{plus,minus}.segments, 1-based,
//                       minus strand emitted in reverse vector order, one lastz command line per file on stdout
//
// Differences by design: std::thread workers instead of a TBB flow graph; the next query block is uploaded by a
// background thread while the current one is processed (the reference's reader lambda does the same through its
// buffer state machine, src/main.cpp:649-685); seeds are generated on the device by default (--host-seeding restores
// the reference's host loop; both give identical files).  Only the engine's C-ABI is used (include/segalign_amd.h).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "segalign_amd.h"
#include "host_common.hpp"

struct Config {  // src/graph.h:32-76 with the defaults of src/main.cpp:61-124
    std::string target, query, data_folder = "./", outdir = ".";
    std::string strand = "both", seed_shape = "12of19", ambiguous = "", scoring_file = "", output_format = "maf-";
    uint32_t step = 1;
    bool transition = true, noentropy = false, gapped = true, notrivial = false, debug = false, host_seeding = false;
    bool gpu_gapped = false;  // --gpu_gapped: a .gapped file next to every .segments file (sa_gapped_extend)
    bool gpu_maf = false;     // --gpu_maf (with --gpu_gapped): a .maf file of the same alignments next to every .gapped file (sa_gapped_align)
    int gpu_pieces = 0;       // --gpu_pieces=N (with --gpu_gapped): engine option gapped_pieces, set before sa_initialize_processor; 0: left alone
    uint32_t gpu_max_extent = 0;  // --gpu_max_extent=N (with --gpu_gapped): sa_gapped_params.max_extent; 0: the engine's default
    bool gpu_skip_covered = false;  // --gpu_skip_covered (with --gpu_gapped): the files hold sa_gapped_align_greedy's alignments
    bool gpu_chain = false;   // --gpu_chain[=diag,anti]: a .chain file next to every .segments file (sa_chain_hsps); the gapped entries get its HSPs only
    int chain_diag = 0, chain_anti = 0;  // sa_chain_params.diag_pen / anti_pen
    uint32_t chain_gap = 0;   // --gpu_chain_gap=N: sa_chain_params.max_gap; 0: unlimited
    bool gpu_chain_all = false;  // --gpu_chain_all[=diag,anti]: a .chains file with all chains (sa_chain_hsps_all); the gapped entries get the kept chains' HSPs
    bool chain_min_set = false;
    long long chain_min = 0;  // --gpu_chain_min=N: sa_chain_params.min_score of --gpu_chain_all
    bool chain_costs_set = false;  // --gpu_chain_costs=loose|medium|FILE (with --gpu_chain or --gpu_chain_all): a piecewise-linear gap cost per link
    sa_chain_gap_costs chain_costs;  // (sa_chain_hsps_costs / sa_chain_hsps_all_costs)
    uint32_t chain_overlap = 0;  // --gpu_chain_overlap[=N] (with --gpu_chain or --gpu_chain_all): chain members may share up to N bases
                                 // (sa_chain_hsps_ovl / sa_chain_hsps_all_ovl) and the chains are trimmed (sa_trim_chains); 0: off
    bool chain_fill = false;  // --gpu_chain_fill[=thresh[,xdrop]] (with --gpu_chain or --gpu_chain_all): the links of the chains, trimmed ones with
                              // --gpu_chain_overlap, are swept for HSPs the seeds missed and filled (sa_fill_chains); a
                              // .filled.chain / .filled.chains file next to every .chain / .chains file, and every later stage takes the filled chains
    int fill_thresh = 3000, fill_xdrop = 910;
    uint32_t fill_side = 0;   // --gpu_chain_fill_side=N: sa_fill_params.max_side
    bool fill_side_set = false;
    bool gpu_stitch = false;  // --gpu_stitch[=max_link] (with --gpu_chain or --gpu_chain_all): a .stitched.maf file next to every .chain / .chains file (sa_stitch_chains)
    uint32_t stitch_max_link = 0;  // sa_stitch_params.max_link; 0: the engine's default
    bool stitch_min_set = false;
    bool gpu_diff = false;    // --gpu_diff[=base] (with --gpu_maf or --gpu_stitch): a .diff file next to every .maf / .stitched.maf / .net.maf file (sa_diff_alignments)
    bool diff_per_base = false;  // --gpu_diff=base: SA_DIFF_PER_BASE
    int stitch_min = INT32_MIN;    // --gpu_stitch_min=N: sa_stitch_params.min_link_score
    bool gpu_net = false;     // --gpu_net[=min_space] (with --gpu_chain_all): a .net file next to every .chains file (sa_net_chains on the target axis)
    uint32_t net_space = 0;   // sa_net_params.min_space; 0: the engine's default
    bool net_fill_set = false;
    uint32_t net_fill = 0;    // --gpu_net_fill=N: sa_net_params.min_fill
    bool gpu_net_class = false;   // --gpu_net_class (with --gpu_net): a .net.class file next to every .net file (sa_net_classify, the query as the other axis)
    bool net_syn = false;         // --gpu_net_syn=...: the synteny filter's thresholds; .net.class and --gpu_net_subset take the kept fills only
    sa_net_class_params net_syn_p = {0, 0, 0, 0, 0, 0};
    bool gpu_net_subset = false;  // --gpu_net_subset (with --gpu_net): a .net.chains file next to every .net file (sa_net_subset), with --gpu_stitch a .net.maf file
    bool gpu_lift = false;        // --gpu_lift=FILE[,num/den] (with --gpu_net_subset): the BED lines of FILE lifted through every .net.chains file (sa_lift_intervals)
    std::string lift_bed;
    sa_lift_params lift_p = {95, 100};
    int gap_open = 400, gap_extend = 30;
    int xdrop = 910, hspthresh = 3000, ydrop = 9430, gappedthresh = -1;
    uint32_t wga_chunk = 250000, lastz_interval = 10000000, seq_block_size = 500000000;
    int num_gpu = -1, num_threads = 0;
    // derived
    std::string shape;
    uint32_t seed_size = 19;
    int kmer_size = 12;
};
static Config cfg;

struct Arena {  // common/DRAM.h: one contiguous buffer per sequence set
    std::string buf;
    std::vector<std::string> chr_name;
    std::vector<size_t> chr_start;
    std::vector<uint32_t> chr_len;
    std::vector<size_t> block_start;
    std::vector<uint32_t> block_len;
};
struct Interval { uint32_t start, end; };

static Arena R, Q;
static std::string Qrc;  // query_rc_DRAM
static std::vector<std::string> rc_chr_name;
static std::vector<size_t> rc_chr_start;
static std::vector<uint32_t> rc_chr_len;
static std::vector<std::vector<Interval>> q_intervals;  // per query block
static int shape_pos[32], shape_weight, transition_pos[32];

static char rc_char(char c) {  // common/ntcoding.cpp:63-105
    switch (c) {
        case 'a': return 't'; case 'A': return 'T'; case 'c': return 'g'; case 'C': return 'G';
        case 'g': return 'c'; case 'G': return 'C'; case 't': return 'a'; case 'T': return 'A';
        default: return c;  // n N & stay; anything else is reported there as "Bad Nt char" -- kept as is here
    }
}

// ---- arenas + plan: src/main.cpp:320-549 -----------------------------------------------------------------------------
static void load_set(const std::string& path, Arena& A, bool is_query, const char* tag) {
    uint32_t block_no = 0, seq_block_len = 0;
    size_t seq_block_start = 0;
    std::vector<uint32_t> block_chrs;
    A.block_start.push_back(0);
    FILE* names = fopen((cfg.outdir + "/" + tag + "_block" + std::to_string(block_no) + ".name").c_str(), "w");
    auto close_block = [&](uint32_t len) {
        A.block_len.push_back(len);
        if (is_query) {
            for (int i = (int)block_chrs.size() - 1; i >= 0; i--) {  // :369-374
                uint32_t c = block_chrs[i];
                rc_chr_name.push_back(A.chr_name[c]);
                rc_chr_start.push_back(2 * seq_block_start + len - A.chr_start[c] - A.chr_len[c]);
                rc_chr_len.push_back(A.chr_len[c]);
            }
            Qrc.resize(seq_block_start + len, 'N');  // RevComp of the block, :381 / :421
            for (uint32_t i = 0; i < len; i++) Qrc[seq_block_start + i] = rc_char(A.buf[seq_block_start + len - 1 - i]);
            std::vector<Interval> iv;  // :383-393
            uint32_t end_pos = len - cfg.seed_size;
            for (uint32_t cur = 0; len > cfg.seed_size && cur < end_pos; cur += cfg.lastz_interval)
                iv.push_back({cur, std::min(end_pos, cur + cfg.lastz_interval)});
            q_intervals.push_back(iv);
        }
    };
    read_fasta(path, [&](const std::string& name, const std::string& seq) {
        fprintf(names, "%s\n", name.c_str());
        uint32_t c = (uint32_t)A.chr_name.size();
        A.chr_name.push_back(name);
        A.chr_start.push_back(A.buf.size());
        A.chr_len.push_back((uint32_t)seq.size());
        block_chrs.push_back(c);
        A.buf += seq;
        seq_block_len += (uint32_t)seq.size();
        if (seq_block_len > cfg.seq_block_size) {  // :359 / :515
            close_block(seq_block_len);
            seq_block_start = A.buf.size();
            A.block_start.push_back(seq_block_start);
            seq_block_len = 0;
            block_chrs.clear();
            block_no++;
            fclose(names);
            names = fopen((cfg.outdir + "/" + tag + "_block" + std::to_string(block_no) + ".name").c_str(), "w");
        } else {
            A.buf += '&';  // :405-409
            seq_block_len += 1;
        }
    });
    if (seq_block_len > 0) close_block(seq_block_len - 1);  // drop the trailing '&', :411-413
    else A.block_start.pop_back();
    fclose(names);
}

// ---- host seeding: common/ntcoding.cpp:43-61 + src/seeder.cpp:57-74 (only with --host-seeding) ----------------------
static uint32_t host_kmer(const char* s, size_t pos) {
    uint32_t code[32];
    for (uint32_t i = 0; i < cfg.seed_size; i++) {
        switch (s[pos + i]) {
            case 'A': code[i] = 0; break; case 'C': code[i] = 1; break;
            case 'G': code[i] = 2; break; case 'T': code[i] = 3; break;
            default: return 1u << 31;
        }
    }
    uint32_t k = 0;
    for (int i = 0; i < shape_weight; i++) k = (k << 2) + code[shape_pos[i]];
    return k;
}

struct Hsps { std::vector<sa_segment_pair> fw, rc; };
static std::atomic<uint64_t> g_num_seed_hits(0), g_num_hsps(0);

// seeder_body::operator(), src/seeder.cpp:12-127
static void seed_interval(size_t q_block_start, uint32_t q_len /* block_len - seed_size */, Interval iv, uint32_t buffer, Hsps& out) {
    for (int rev = 0; rev < 2; rev++) {
        if (rev == 0 && !(cfg.strand == "plus" || cfg.strand == "both")) continue;
        if (rev == 1 && !(cfg.strand == "minus" || cfg.strand == "both")) continue;
        uint32_t a = rev ? q_len - iv.end : iv.start, b = rev ? q_len - iv.start : iv.end;  // :33-34
        std::vector<sa_segment_pair>& dst = rev ? out.rc : out.fw;
        if (!cfg.host_seeding) {
            // device seeding: up to sa_max_chunks_per_call() consecutive chunks share one pass over the kernels; every
            // chunk still gets its own return vector, identical to one call per chunk
            const int kmax = sa_get_chunks_per_call();  // (chunks_per_call, or more when the resident target's seed hits are sparse)
            std::vector<sa_segment_pair*> res((size_t)kmax, nullptr);
            std::vector<size_t> n((size_t)kmax, 0);
            for (uint64_t i = a; i < b; i += (uint64_t)cfg.wga_chunk * kmax) {
                const uint32_t e = (uint32_t)std::min<uint64_t>(i + (uint64_t)cfg.wga_chunk * kmax, b);
                const int nc = (int)((e - i + cfg.wga_chunk - 1) / cfg.wga_chunk);  // chunks of THIS call: only their slots are written
                sa_seed_and_filter_chunks((uint32_t)i, e, rev, buffer, res.data(), n.data());
                for (int c = 0; c < nc; c++) {
                    if (!n[c]) continue;
                    g_num_seed_hits += (uint32_t)res[c][0].score;
                    if (n[c] > 1) {
                        dst.insert(dst.end(), res[c] + 1, res[c] + n[c]);
                        g_num_hsps += n[c] - 1;
                    }
                    sa_free_segments(res[c]);
                }
            }
            continue;
        }
        for (uint32_t i = a; i < b; i += cfg.wga_chunk) {  // the reference's loop: seed words built on the host, :57-74
            uint32_t e = std::min(i + cfg.wga_chunk, b);
            sa_segment_pair* res = nullptr;
            size_t n = 0;
            const std::string& buf = rev ? Qrc : Q.buf;
            std::vector<uint64_t> seeds;
            for (uint32_t j = i; j < e; j++) {
                uint64_t k = host_kmer(buf.data(), q_block_start + j);
                if (k != (1u << 31)) {
                    seeds.push_back((k << 32) + j);
                    if (cfg.transition)
                        for (int t = 0; t < shape_weight; t++)
                            if (transition_pos[t]) seeds.push_back(((k ^ ((uint64_t)2 << (2 * t))) << 32) + j);
                }
            }
            if (!seeds.empty()) n = sa_seed_and_filter(seeds.data(), seeds.size(), rev, buffer, &res);
            if (n) {
                g_num_seed_hits += (uint32_t)res[0].score;
                if (n > 1) {
                    dst.insert(dst.end(), res + 1, res + n);
                    g_num_hsps += n - 1;
                }
                sa_free_segments(res);
            }
        }
    }
}

// ---- --gpu_lift: the BED file, read once ----
struct BedLine {
    std::string line;  // as read, without its line end
    std::string rest;  // what follows the third field, its tab included
    long record;       // index of the target record named in the first field, -1: none of the target's
    uint64_t start, end;
};
static std::vector<BedLine> bed_lines;

static void load_bed(const std::string& path) {
    FILE* f = fopen(path.c_str(), "r");
    if (!f) die(7, "cant open file: %s", path.c_str());
    std::string line;
    size_t no = 0;
    for (int ch = 0; ch != EOF;) {
        line.clear();
        while ((ch = fgetc(f)) != EOF && ch != '\n') line.push_back((char)ch);
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (ch == EOF && line.empty()) break;
        no++;
        if (line.empty() || line[0] == '#') continue;
        BedLine b;
        const size_t t1 = line.find('\t'), t2 = t1 == std::string::npos ? t1 : line.find('\t', t1 + 1);
        char* endp = nullptr;
        bool ok = t2 != std::string::npos;
        if (ok) {
            b.start = strtoull(line.c_str() + t1 + 1, &endp, 10);
            ok = endp == line.c_str() + t2 && t2 > t1 + 1;
        }
        size_t t3 = std::string::npos;
        if (ok) {
            b.end = strtoull(line.c_str() + t2 + 1, &endp, 10);
            t3 = (size_t)(endp - line.c_str());
            ok = t3 > t2 + 1 && (t3 == line.size() || line[t3] == '\t') && b.start < b.end;
        }
        if (!ok) {
            fprintf(stderr, "--gpu_lift: %s line %zu is no BED line (name, start, end with start < end, tab-separated)\n", path.c_str(), no);
            exit(1);
        }
        b.line = line;
        b.rest = line.substr(t3);
        const std::string name = line.substr(0, t1);
        b.record = -1;
        for (size_t c = 0; c < R.chr_name.size() && b.record < 0; c++)
            if (R.chr_name[c] == name) b.record = (long)c;
        bed_lines.push_back(b);
    }
    fclose(f);
}

static size_t chr_of(const std::vector<size_t>& starts, size_t pos) {
    return (size_t)(std::upper_bound(starts.begin(), starts.end(), pos) - starts.begin()) - 1;
}
static std::mutex io_lock;

// segment_printer_body::operator(), src/segment_printer.cpp:11-173
static void print_segments(int r_block_index, int q_block_index, size_t r_block_start, size_t q_block_start, uint32_t index,
                           const Hsps& h, uint32_t buffer) {
    for (int rev = 0; rev < 2; rev++) {
        const std::vector<sa_segment_pair>& v = rev ? h.rc : h.fw;
        if (v.empty()) continue;
        const std::vector<std::string>& qn = rev ? rc_chr_name : Q.chr_name;
        const std::vector<size_t>& qs = rev ? rc_chr_start : Q.chr_start;
        std::string base = "tmp" + std::to_string(index) + ".block" + std::to_string(q_block_index) + ".r" +
                           std::to_string(r_block_start) + (rev ? ".minus" : ".plus");
        std::string seg_name = base + ".segments";
        FILE* f = fopen((cfg.outdir + "/" + seg_name).c_str(), "w");
        if (!f) die(7, "cant open file: %s", seg_name.c_str());
        auto emit = [&](const sa_segment_pair& e) {
            size_t seg_r = e.ref_start + r_block_start, seg_q = e.query_start + q_block_start;
            size_t ri = chr_of(R.chr_start, seg_r), qi = chr_of(qs, seg_q);
            fprintf(f, "%s\t%zu\t%zu\t%s\t%zu\t%zu\t%c\t%d\n", R.chr_name[ri].c_str(), seg_r + 1 - R.chr_start[ri],
                    seg_r + e.len + 1 - R.chr_start[ri], qn[qi].c_str(), seg_q + 1 - qs[qi], seg_q + e.len + 1 - qs[qi],
                    rev ? '-' : '+', e.score);
        };
        if (!rev) for (size_t i = 0; i < v.size(); i++) emit(v[i]);
        else for (size_t i = v.size(); i-- > 0;) emit(v[i]);  // :130: reverse vector order on the minus strand
        fclose(f);
        // with --gpu_diff: the differences of a .maf file's alignments into the file dname, in the .maf file's order:
        // the spans in their order, or backwards
        auto write_diff = [&](const std::string& dname, const std::vector<sa_diff_span>& spans, const uint32_t* dops, size_t n_dops, bool backwards) {
            const sa_diff_params dp = {cfg.diff_per_base ? SA_DIFF_PER_BASE : 0u, 0};
            sa_diff_event* ev = nullptr;
            sa_diff_summary* sm = nullptr;
            sa_diff_alignments(spans.data(), spans.size(), dops, n_dops, rev, buffer, &dp, &ev, &sm, nullptr);
            FILE* df = fopen((cfg.outdir + "/" + dname).c_str(), "w");
            if (!df) die(7, "cant open file: %s", dname.c_str());
            const std::string& qbuf = rev ? Qrc : Q.buf;
            static const char* const kind_name[4] = {"sub", "other", "ins", "del"};
            for (size_t x = 0; x < spans.size(); x++) {
                const size_t k = backwards ? spans.size() - 1 - x : x;
                const sa_diff_summary& m = sm[k];
                const size_t r0 = spans[k].ref_start + r_block_start, q0 = spans[k].query_start + q_block_start;
                const size_t ri = chr_of(R.chr_start, r0), qi = chr_of(qs, q0);
                fprintf(df, "#a %zu %s %zu %s %c %zu columns=%u matches=%u transitions=%u transversions=%u others=%u ins=%u/%u del=%u/%u events=%u identity=%u/%u\n",
                        x, R.chr_name[ri].c_str(), r0 - R.chr_start[ri], qn[qi].c_str(), rev ? '-' : '+', q0 - qs[qi], m.columns, m.matches,
                        m.transitions, m.transversions, m.others, m.ins_runs, m.ins_bases, m.del_runs, m.del_bases, m.n_events, m.matches, m.columns);
                for (uint64_t e = m.first_event; e < m.first_event + m.n_events; e++) {
                    const sa_diff_event& d = ev[e];
                    const size_t r = d.ref_pos + r_block_start, q = d.query_pos + q_block_start;
                    fprintf(df, "%s\t%s\t%zu\t%s\t%c\t%zu\t%u\t%c\t%c\n", kind_name[d.kind], R.chr_name[ri].c_str(), r - R.chr_start[ri], qn[qi].c_str(),
                            rev ? '-' : '+', q - qs[qi], d.len, d.kind == SA_DIFF_INS ? '-' : R.buf[r], d.kind == SA_DIFF_DEL ? '-' : qbuf[q]);
                }
            }
            fclose(df);
            sa_free_diff(ev, sm);
        };
        std::vector<sa_segment_pair> kept;  // with --gpu_chain or --gpu_chain_all: the chains' HSPs in their order within v
        if (cfg.gpu_chain || cfg.gpu_chain_all) {  // chains within every (target record, query record) pair of this file, DESIGN.md 15 and 16
            const char* flag = cfg.gpu_chain ? "--gpu_chain" : "--gpu_chain_all";
            if (v.size() > ((size_t)1 << 22))  // sa_chain_hsps' limit, told in the host's words
            {
                fprintf(stderr, "%s: %s holds %zu HSPs, more than the 4194304 one chaining call takes; lower --lastz_interval\n", flag, seg_name.c_str(), v.size());
                exit(8);
            }
            std::vector<uint64_t> rec_pair(v.size());
            for (size_t i = 0; i < v.size(); i++)
                rec_pair[i] = (uint64_t)chr_of(R.chr_start, v[i].ref_start + r_block_start) << 32 | (uint64_t)chr_of(qs, v[i].query_start + q_block_start);
            std::vector<uint64_t> pairs(rec_pair);  // group = rank of the pair among the file's pairs: ascending (target record, query record)
            std::sort(pairs.begin(), pairs.end());
            pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
            std::vector<uint32_t> group(v.size());
            for (size_t i = 0; i < v.size(); i++) group[i] = (uint32_t)(std::lower_bound(pairs.begin(), pairs.end(), rec_pair[i]) - pairs.begin());
            sa_chain_params cp = {cfg.chain_diag, cfg.chain_anti, cfg.chain_gap, 0, cfg.gpu_chain_all ? (int64_t)cfg.chain_min : 0};
            std::string cname = base + (cfg.gpu_chain ? ".chain" : ".chains");
            f = fopen((cfg.outdir + "/" + cname).c_str(), "w");
            if (!f) die(7, "cant open file: %s", cname.c_str());
            std::vector<uint32_t> idx, cfirst(1, 0);  // cfirst: the chains' offsets into the members, for --gpu_stitch and --gpu_net
            std::vector<int64_t> cscore;              // with --gpu_net: every kept chain's score and the target record of its pair
            std::vector<uint32_t> ctarget;
            std::vector<uint32_t> cquery;             // with --gpu_net_class: the query record of its pair
            const sa_chain_gap_costs* costs = cfg.chain_costs_set ? &cfg.chain_costs : nullptr;
            const sa_chain_overlap ov = {cfg.chain_overlap, 0};
            std::vector<sa_chain_record> crec;        // with --gpu_chain_all: the kept chains' records
            if (cfg.gpu_chain) {
                sa_chain_member* mem = nullptr;
                const size_t nm = cfg.chain_overlap ? sa_chain_hsps_ovl(v.data(), v.size(), group.data(), &cp, costs, &ov, &mem, nullptr, nullptr)
                                : cfg.chain_costs_set ? sa_chain_hsps_costs(v.data(), v.size(), group.data(), &cp, &cfg.chain_costs, &mem, nullptr, nullptr)
                                                      : sa_chain_hsps(v.data(), v.size(), group.data(), &cp, &mem, nullptr, nullptr);
                idx.resize(nm);
                for (size_t k = 0; k < nm; k++) idx[k] = mem[k].hsp_index;  // the order sa_chain_hsps returns, on both strands
                for (size_t k = 1; k <= nm; k++)
                    if (k == nm || mem[k].group != mem[k - 1].group) cfirst.push_back((uint32_t)k);  // one chain per group
                sa_free_chain(mem, nullptr);
            } else {
                sa_chain_record* ch = nullptr;
                sa_chain_all_member* mem = nullptr;
                size_t nc = 0;
                const size_t nm = cfg.chain_overlap
                    ? sa_chain_hsps_all_ovl(v.data(), v.size(), group.data(), &cp, costs, &ov, &ch, &nc, &mem, nullptr, nullptr, nullptr)
                    : cfg.chain_costs_set
                    ? sa_chain_hsps_all_costs(v.data(), v.size(), group.data(), &cp, &cfg.chain_costs, &ch, &nc, &mem, nullptr, nullptr, nullptr)
                    : sa_chain_hsps_all(v.data(), v.size(), group.data(), &cp, &ch, &nc, &mem, nullptr, nullptr, nullptr);
                idx.resize(nm);
                crec.assign(ch, ch + nc);
                for (size_t c = 0; c < nc; c++) {
                    for (size_t k = ch[c].first_member; k < (size_t)ch[c].first_member + ch[c].n_members; k++) idx[k] = mem[k].hsp_index;
                    cfirst.push_back(ch[c].first_member + ch[c].n_members);  // the chains' members follow one another
                }
                sa_free_chain_all(ch, mem, nullptr, nullptr);
            }
            // with --gpu_chain_overlap the members may overlap: cut every overlap at the best crossover.  From here on the
            // chains' HSP vector is the trimmed one, one entry per member, and the chains' scores are the exact ones
            std::vector<sa_segment_pair> trimmed;
            std::vector<uint32_t> untrimmed_idx;  // the members' indices in v
            if (cfg.chain_overlap) {
                sa_segment_pair* th = nullptr;
                sa_trim_chain* tc = nullptr;
                const size_t tm = sa_trim_chains(v.data(), v.size(), idx.data(), cfirst.data(), cfirst.size() - 1, rev, buffer, &cp, costs, 0, &th, &tc,
                                                 nullptr, nullptr, nullptr);
                trimmed.assign(th, th + tm);
                for (size_t c = 0; c < crec.size(); c++) crec[c].score = tc[c].score;
                sa_free_trim(th, tc, nullptr);
                untrimmed_idx = idx;
                for (size_t k = 0; k < idx.size(); k++) idx[k] = (uint32_t)k;
            }
            auto write_chains = [&](const std::vector<sa_segment_pair>& hv) {  // the chains of idx, cfirst and crec over hv, into f
                if (cfg.gpu_chain) {
                    for (size_t k = 0; k < idx.size(); k++) emit(hv[idx[k]]);
                } else {
                    for (size_t c = 0; c < crec.size(); c++) {  // the order sa_chain_hsps_all returns, on both strands
                        fprintf(f, "#chain %zu group=%u score=%lld members=%u joined=%d\n", c, crec[c].group, (long long)crec[c].score, crec[c].n_members,
                                crec[c].joined >= 0 ? 1 : 0);
                        for (size_t k = crec[c].first_member; k < (size_t)crec[c].first_member + crec[c].n_members; k++) emit(hv[idx[k]]);
                    }
                }
            };
            write_chains(cfg.chain_overlap ? trimmed : v);
            fclose(f);
            // with --gpu_chain_fill the space between consecutive members is swept for what the seeds missed.  From here on
            // the chains' HSP vector is the filled one, one entry per member or fill, and the chains' scores are the filled chains'
            std::vector<sa_segment_pair> filled;
            std::vector<uint32_t> fill_vkey;  // per entry: the index in v of the member it is, or of the member its fill follows
            if (cfg.chain_fill) {
                const std::vector<sa_segment_pair>& hv = cfg.chain_overlap ? trimmed : v;
                const sa_fill_params fp = {cfg.fill_thresh, cfg.fill_xdrop, cfg.fill_side, 0, 0, 0};
                sa_segment_pair* fh = nullptr;
                uint32_t *ffirst = nullptr, *forigin = nullptr;
                sa_fill_chain* fc = nullptr;
                const size_t fe = sa_fill_chains(hv.data(), hv.size(), idx.data(), cfirst.data(), cfirst.size() - 1, rev, buffer, &cp, costs, &fp, 0, &fh,
                                                 &ffirst, &forigin, &fc, nullptr, nullptr, nullptr, nullptr, nullptr);
                filled.assign(fh, fh + fe);
                fill_vkey.resize(fe);
                for (size_t k = 0; k < fe; k++)
                    fill_vkey[k] = forigin[k] == SA_FILL_NONE ? fill_vkey[k - 1] : cfg.chain_overlap ? untrimmed_idx[forigin[k]] : forigin[k];
                for (size_t c = 0; c + 1 < cfirst.size(); c++) cfirst[c + 1] = ffirst[c + 1];
                for (size_t c = 0; c < crec.size(); c++) {
                    crec[c].score = fc[c].score;
                    crec[c].first_member = cfirst[c];
                    crec[c].n_members = cfirst[c + 1] - cfirst[c];
                }
                sa_free_fill(fh, ffirst, forigin, fc, nullptr, nullptr);
                idx.resize(fe);
                for (size_t k = 0; k < fe; k++) idx[k] = (uint32_t)k;
                std::string fname = base + (cfg.gpu_chain ? ".filled.chain" : ".filled.chains");
                f = fopen((cfg.outdir + "/" + fname).c_str(), "w");
                if (!f) die(7, "cant open file: %s", fname.c_str());
                write_chains(filled);
                fclose(f);
            }
            const std::vector<sa_segment_pair>& cv = cfg.chain_fill ? filled : cfg.chain_overlap ? trimmed : v;  // what idx indexes
            if (cfg.gpu_net)
                for (size_t c = 0; c < crec.size(); c++) {
                    cscore.push_back(crec[c].score);
                    ctarget.push_back((uint32_t)(pairs[crec[c].group] >> 32));
                    cquery.push_back((uint32_t)pairs[crec[c].group]);
                }
            // every chain of a CSR as one alignment through its members, in --gpu_maf's block layout, into the file sname
            auto write_stitched = [&](const std::string& sname, const sa_segment_pair* sh, size_t n_sh, const uint32_t* smem, const uint32_t* sfirst,
                                      size_t n_sc) {
                sa_stitch_params sp = {cfg.gap_open, cfg.gap_extend, cfg.stitch_max_link, cfg.stitch_min};
                sa_stitch_record* sr = nullptr;
                uint32_t* sops = nullptr;
                size_t n_sops = 0;
                const size_t ns = sa_stitch_chains(sh, n_sh, smem, sfirst, n_sc, rev, buffer, &sp, &sr, &sops, &n_sops, nullptr, nullptr, nullptr);
                FILE* sf = fopen((cfg.outdir + "/" + sname).c_str(), "w");
                if (!sf) die(7, "cant open file: %s", sname.c_str());
                const std::string& qbuf = rev ? Qrc : Q.buf;
                const std::vector<uint32_t>& ql = rev ? rc_chr_len : Q.chr_len;
                for (size_t k = 0; k < ns; k++) {  // the order sa_stitch_chains returns, on both strands, as the .chain files
                    const sa_stitch_record& a = sr[k];
                    size_t r0 = a.ref_start + r_block_start, q0 = a.query_start + q_block_start;
                    size_t ri = chr_of(R.chr_start, r0), qi = chr_of(qs, q0);
                    std::string ta, qa;
                    size_t i = r0, j = q0;
                    for (size_t x = a.op_offset; x < a.op_offset + a.n_ops; x++) {
                        const size_t len = sops[x] >> 2, op = sops[x] & 3u;
                        if (op == SA_GAPPED_OP_I) ta.append(len, '-');
                        else { ta.append(R.buf, i, len); i += len; }
                        if (op == SA_GAPPED_OP_D) qa.append(len, '-');
                        else { qa.append(qbuf, j, len); j += len; }
                    }
                    fprintf(sf, "a score=%lld\n", (long long)a.score);
                    fprintf(sf, "s %s %zu %u + %u %s\n", R.chr_name[ri].c_str(), r0 - R.chr_start[ri], a.ref_end - a.ref_start, R.chr_len[ri], ta.c_str());
                    fprintf(sf, "s %s %zu %u %c %u %s\n\n", qn[qi].c_str(), q0 - qs[qi], a.query_end - a.query_start, rev ? '-' : '+', ql[qi],
                            qa.c_str());
                }
                fclose(sf);
                if (cfg.gpu_diff) {
                    std::vector<sa_diff_span> spans(ns);
                    for (size_t k = 0; k < ns; k++) spans[k] = {sr[k].ref_start, sr[k].query_start, sr[k].op_offset, sr[k].n_ops, 0};
                    write_diff(sname.substr(0, sname.size() - 3) + "diff", spans, sops, n_sops, false);
                }
                sa_free_stitch(sr, sops, nullptr);
            };
            if (cfg.gpu_stitch) write_stitched(base + ".stitched.maf", cv.data(), cv.size(), idx.data(), cfirst.data(), cfirst.size() - 1);
            if (cfg.gpu_net) {  // which chain to believe where: the kept chains of every target record netted on the target axis
                std::vector<uint32_t> bs(idx.size()), be(idx.size());  // a member is one block, in block coordinates
                for (size_t k = 0; k < idx.size(); k++) {
                    bs[k] = cv[idx[k]].ref_start;
                    be[k] = cv[idx[k]].ref_start + cv[idx[k]].len + 1;
                }
                sa_net_params np = {cfg.net_space, cfg.net_fill};
                sa_net_fill* nf = nullptr;
                const size_t nn = sa_net_chains(cfirst.data(), bs.data(), be.data(), cscore.data(), ctarget.data(), cfirst.size() - 1, &np, &nf, nullptr);
                // where every fill lands on the query relative to its parent, and what it shares there with other fills; a
                // file holds one strand, so every chain has ostrand 0 and the coordinates go in as they are
                sa_net_class* ncl = nullptr;
                FILE* cfp = nullptr;
                if (cfg.gpu_net_class) {
                    std::vector<uint32_t> obs(idx.size()), obe(idx.size());
                    for (size_t k = 0; k < idx.size(); k++) {
                        obs[k] = cv[idx[k]].query_start;
                        obe[k] = cv[idx[k]].query_start + cv[idx[k]].len + 1;
                    }
                    sa_net_classify(cfirst.data(), bs.data(), be.data(), obs.data(), obe.data(), cquery.data(), nullptr, cfirst.size() - 1, nf, nn,
                                    cfg.net_syn ? &cfg.net_syn_p : nullptr, cfg.net_syn ? SA_NETCLASS_FILTER : 0, &ncl, nullptr);
                    std::string class_name = base + ".net.class";
                    cfp = fopen((cfg.outdir + "/" + class_name).c_str(), "w");
                    if (!cfp) die(7, "cant open file: %s", class_name.c_str());
                }
                bool class_head = false;  // this record's net line stands in the .net.class file
                std::string nname = base + ".net";
                FILE* nfp = fopen((cfg.outdir + "/" + nname).c_str(), "w");
                if (!nfp) die(7, "cant open file: %s", nname.c_str());
                for (size_t k = 0; k < nn; k++) {  // the order sa_net_chains returns: by target record, then the pre-order walk of its net
                    const sa_net_fill& x = nf[k];
                    const size_t ri = x.group;
                    if (k == 0 || nf[k - 1].group != x.group) {
                        fprintf(nfp, "net %s %u\n", R.chr_name[ri].c_str(), R.chr_len[ri]);
                        class_head = false;
                    }
                    // an HSP is ungapped: a clip on the target shifts the query by the same amount
                    const uint32_t k0 = x.first_block, k1 = x.first_block + x.n_blocks - 1;
                    const size_t q0 = (size_t)cv[idx[k0]].query_start + (x.start - bs[k0]) + q_block_start;
                    const size_t q1 = (size_t)cv[idx[k1]].query_start + (x.end - bs[k1]) + q_block_start;
                    const size_t qi = chr_of(qs, q0);
                    fprintf(nfp, "%*sfill %zu %u %s %c %zu %zu chain=%u score=%lld ali=%u\n", (int)x.depth, "", x.start + r_block_start - R.chr_start[ri],
                            x.end - x.start, qn[qi].c_str(), rev ? '-' : '+', q0 - qs[qi], q1 - q0, x.chain, (long long)x.score, x.ali);
                    if (cfp && ncl[k].keep) {  // the same line and the class; a record's net line before its first kept fill
                        static const char* const type_name[4] = {"top", "syn", "inv", "nonSyn"};
                        if (!class_head) fprintf(cfp, "net %s %u\n", R.chr_name[ri].c_str(), R.chr_len[ri]);
                        class_head = true;
                        fprintf(cfp, "%*sfill %zu %u %s %c %zu %zu chain=%u score=%lld ali=%u type=%s qover=%u qfar=%u qdup=%u\n", (int)x.depth, "",
                                x.start + r_block_start - R.chr_start[ri], x.end - x.start, qn[qi].c_str(), rev ? '-' : '+', q0 - qs[qi], q1 - q0, x.chain,
                                (long long)x.score, x.ali, type_name[ncl[k].type & 3], ncl[k].oover, ncl[k].ofar, ncl[k].odup);
                    }
                }
                fclose(nfp);
                if (cfp) fclose(cfp);
                std::vector<sa_net_fill> kept_fills;  // with --gpu_net_syn: the kept fills as a net of their own, parents renumbered
                const sa_net_fill* sub_fills = nf;
                size_t n_sub_fills = nn;
                if (cfg.net_syn) {
                    std::vector<int32_t> renum(nn, -1);
                    for (size_t k = 0; k < nn; k++) {
                        if (!ncl[k].keep) continue;
                        sa_net_fill x = nf[k];
                        if (x.parent >= 0) x.parent = renum[x.parent];  // keep is closed under subtrees: the parent is kept
                        renum[k] = (int32_t)kept_fills.size();
                        kept_fills.push_back(x);
                    }
                    sub_fills = kept_fills.data();
                    n_sub_fills = kept_fills.size();
                }
                sa_free_net_class(ncl);
                if (cfg.gpu_net_subset) {  // every fill's part of its chain as a chain of its own, under the penalties of --gpu_chain_all
                    sa_segment_pair* oh = nullptr;
                    sa_subset_chain* sc = nullptr;
                    size_t n_oh = 0;
                    const size_t nsc = sa_net_subset(cv.data(), cv.size(), idx.data(), cfirst.data(), cfirst.size() - 1, sub_fills, n_sub_fills, 0, rev, buffer, &cp,
                                                     cfg.chain_costs_set ? &cfg.chain_costs : nullptr, SA_SUBSET_SPLIT, &oh, &n_oh, &sc, nullptr);
                    std::string sname = base + ".net.chains";
                    f = fopen((cfg.outdir + "/" + sname).c_str(), "w");
                    if (!f) die(7, "cant open file: %s", sname.c_str());
                    std::vector<uint32_t> smem(n_oh), sfirst(1, 0);
                    for (size_t k = 0; k < n_oh; k++) smem[k] = (uint32_t)k;
                    for (size_t c = 0; c < nsc; c++) {  // the order sa_net_subset returns: by fill, then by run
                        const sa_subset_chain& x = sc[c];
                        const size_t r0 = x.ref_start + r_block_start, q0 = x.query_start + q_block_start;
                        const size_t ri = chr_of(R.chr_start, r0), qi = chr_of(qs, q0);
                        fprintf(f, "#chain %zu fill=%u run=%u score=%lld %s %zu %zu %s %zu %zu %c\n", c, x.fill, x.run, (long long)x.score,
                                R.chr_name[ri].c_str(), r0 + 1 - R.chr_start[ri], x.ref_end + r_block_start - R.chr_start[ri], qn[qi].c_str(),
                                q0 + 1 - qs[qi], x.query_end + q_block_start - qs[qi], rev ? '-' : '+');
                        for (size_t k = x.first_member; k < (size_t)x.first_member + x.n_members; k++) emit(oh[k]);
                        sfirst.push_back(x.first_member + x.n_members);
                    }
                    fclose(f);
                    if (cfg.gpu_stitch) write_stitched(base + ".net.maf", oh, n_oh, smem.data(), sfirst.data(), nsc);
                    if (cfg.gpu_lift) {  // the BED lines inside this target block through the sub-chains, the query as the other axis
                        const size_t r_block_end = r_block_start + R.block_len[r_block_index];
                        std::vector<uint32_t> lbs(n_oh), lbe(n_oh), lobs(n_oh), lobe(n_oh), lgroup(nsc), logroup(nsc), ivg, ivs, ive;
                        std::vector<size_t> which;  // the lines lifted here
                        for (size_t k = 0; k < n_oh; k++) {
                            lbs[k] = oh[k].ref_start;
                            lbe[k] = oh[k].ref_start + oh[k].len + 1;
                            lobs[k] = oh[k].query_start;
                            lobe[k] = oh[k].query_start + oh[k].len + 1;
                        }
                        for (size_t c = 0; c < nsc; c++) {
                            lgroup[c] = (uint32_t)chr_of(R.chr_start, sc[c].ref_start + r_block_start);
                            logroup[c] = (uint32_t)chr_of(qs, sc[c].query_start + q_block_start);
                        }
                        for (size_t k = 0; k < bed_lines.size(); k++) {
                            const BedLine& b = bed_lines[k];
                            if (b.record < 0 || b.end > R.chr_len[b.record]) continue;
                            const size_t s = R.chr_start[b.record] + b.start, e = R.chr_start[b.record] + b.end;
                            if (s < r_block_start || e > r_block_end) continue;
                            which.push_back(k);
                            ivg.push_back((uint32_t)b.record);
                            ivs.push_back((uint32_t)(s - r_block_start));
                            ive.push_back((uint32_t)(e - r_block_start));
                        }
                        sa_lift_record* lr = nullptr;
                        sa_lift_hit* lh = nullptr;
                        sa_lift_block* lb = nullptr;
                        size_t n_lh = 0, n_lb = 0;
                        sa_lift_intervals(sfirst.data(), lbs.data(), lbe.data(), lobs.data(), lobe.data(), lgroup.data(), logroup.data(), nullptr, nsc,
                                          ivg.data(), ivs.data(), ive.data(), which.size(), &cfg.lift_p, 0, &lr, &lh, &n_lh, &lb, &n_lb, nullptr);
                        std::string lname = base + ".lifted.bed", uname = base + ".unlifted.bed";
                        FILE* lf = fopen((cfg.outdir + "/" + lname).c_str(), "w");
                        if (!lf) die(7, "cant open file: %s", lname.c_str());
                        FILE* uf = fopen((cfg.outdir + "/" + uname).c_str(), "w");
                        if (!uf) die(7, "cant open file: %s", uname.c_str());
                        static const char* const reason[4] = {"#Deleted", "#Partially deleted", "", "#Duplicated"};
                        for (size_t k = 0; k < which.size(); k++) {
                            const BedLine& b = bed_lines[which[k]];
                            const sa_lift_record& x = lr[k];
                            if (x.status == SA_LIFT_MAPPED) {
                                const size_t qi = x.ogroup;
                                fprintf(lf, "%s\t%zu\t%zu%s\t%c\n", qn[qi].c_str(), x.ostart + q_block_start - qs[qi], x.oend + q_block_start - qs[qi],
                                        b.rest.c_str(), rev ? '-' : '+');
                            } else {
                                fprintf(uf, "%s\n%s\n", reason[x.status & 3], b.line.c_str());
                            }
                        }
                        fclose(lf);
                        fclose(uf);
                        sa_free_lift(lr, lh, lb);
                    }
                    sa_free_net_subset(oh, sc);
                }
                sa_free_net(nf);
            }
            kept.reserve(idx.size());
            if (cfg.chain_fill) {  // the members in the order of their HSPs within v, every fill behind the member it follows
                std::vector<uint32_t> ord(idx);
                std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return fill_vkey[x] < fill_vkey[y]; });
                for (uint32_t k : ord) kept.push_back(filled[k]);
            } else if (cfg.chain_overlap) {  // the trimmed members in the order of their HSPs within v
                std::vector<uint32_t> ord(idx);
                std::sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return untrimmed_idx[x] < untrimmed_idx[y]; });
                for (uint32_t k : ord) kept.push_back(trimmed[k]);
            } else {
                std::sort(idx.begin(), idx.end());  // an HSP is a member of one chain at most: no duplicates
                for (uint32_t i : idx) kept.push_back(v[i]);
            }
        }
        const std::vector<sa_segment_pair>& anchors = (cfg.gpu_chain || cfg.gpu_chain_all) ? kept : v;  // what the gapped entries extend
        if (cfg.gpu_gapped) {  // the gapped extension of the same HSPs on the device: [start, end) extents printed like the segments
            sa_gapped_params gp = {cfg.gap_open, cfg.gap_extend, cfg.ydrop, cfg.gappedthresh, cfg.gpu_max_extent, 0};
            sa_gapped_alignment* al = nullptr;
            sa_gapped_path* paths = nullptr;
            uint32_t* ops = nullptr;
            size_t n_ops = 0;
            const bool with_paths = cfg.gpu_maf || cfg.gpu_skip_covered;
            const size_t na = cfg.gpu_skip_covered ? sa_gapped_align_greedy(anchors.data(), anchors.size(), rev, buffer, &gp, &al, &paths, &ops, &n_ops, nullptr)
                              : cfg.gpu_maf        ? sa_gapped_align(anchors.data(), anchors.size(), rev, buffer, &gp, 0, &al, &paths, &ops, &n_ops, nullptr)
                                                   : sa_gapped_extend(anchors.data(), anchors.size(), rev, buffer, &gp, 0, &al, nullptr);
            std::string gname = base + ".gapped";
            FILE* g = fopen((cfg.outdir + "/" + gname).c_str(), "w");
            if (!g) die(7, "cant open file: %s", gname.c_str());
            auto emit_gapped = [&](const sa_gapped_alignment& a) {
                size_t r0 = a.ref_start + r_block_start, q0 = a.query_start + q_block_start;
                size_t ri = chr_of(R.chr_start, r0), qi = chr_of(qs, q0);
                fprintf(g, "%s\t%zu\t%zu\t%s\t%zu\t%zu\t%c\t%d\n", R.chr_name[ri].c_str(), r0 + 1 - R.chr_start[ri],
                        a.ref_end + r_block_start - R.chr_start[ri], qn[qi].c_str(), q0 + 1 - qs[qi], a.query_end + q_block_start - qs[qi],
                        rev ? '-' : '+', a.score);
            };
            if (!rev) for (size_t i = 0; i < na; i++) emit_gapped(al[i]);
            else for (size_t i = na; i-- > 0;) emit_gapped(al[i]);  // reverse order on the minus strand, as the segments
            fclose(g);
            if (cfg.gpu_maf) {  // LASTZ's maf- blocks (no header): 0-based starts within the record, minus-strand query in rc coordinates
                std::string mname = base + ".maf";
                FILE* mf = fopen((cfg.outdir + "/" + mname).c_str(), "w");
                if (!mf) die(7, "cant open file: %s", mname.c_str());
                const std::string& qbuf = rev ? Qrc : Q.buf;
                const std::vector<uint32_t>& ql = rev ? rc_chr_len : Q.chr_len;
                auto emit_maf = [&](size_t k) {
                    const sa_gapped_alignment& a = al[k];
                    const sa_gapped_path& p = paths[k];
                    size_t r0 = a.ref_start + r_block_start, q0 = a.query_start + q_block_start;
                    size_t ri = chr_of(R.chr_start, r0), qi = chr_of(qs, q0);
                    std::string ta, qa;
                    size_t i = r0, j = q0;
                    for (size_t x = p.op_offset; x < p.op_offset + p.n_left + p.n_right; x++) {
                        const size_t len = ops[x] >> 2, op = ops[x] & 3u;
                        if (op == SA_GAPPED_OP_I) ta.append(len, '-');
                        else { ta.append(R.buf, i, len); i += len; }
                        if (op == SA_GAPPED_OP_D) qa.append(len, '-');
                        else { qa.append(qbuf, j, len); j += len; }
                    }
                    fprintf(mf, "a score=%d\n", a.score);
                    fprintf(mf, "s %s %zu %u + %u %s\n", R.chr_name[ri].c_str(), r0 - R.chr_start[ri], a.ref_end - a.ref_start, R.chr_len[ri],
                            ta.c_str());
                    fprintf(mf, "s %s %zu %u %c %u %s\n\n", qn[qi].c_str(), q0 - qs[qi], a.query_end - a.query_start, rev ? '-' : '+', ql[qi],
                            qa.c_str());
                };
                if (!rev) for (size_t k = 0; k < na; k++) emit_maf(k);
                else for (size_t k = na; k-- > 0;) emit_maf(k);  // the .gapped file's order
                fclose(mf);
                if (cfg.gpu_diff) {
                    std::vector<sa_diff_span> spans(na);
                    for (size_t k = 0; k < na; k++) spans[k] = {al[k].ref_start, al[k].query_start, paths[k].op_offset, paths[k].n_left + paths[k].n_right, 0};
                    write_diff(base + ".diff", spans, ops, n_ops, rev != 0);
                }
            }
            if (with_paths) sa_free_gapped_align(al, paths, ops);
            else sa_free_gapped(al);
        }
        if (cfg.gapped) {  // :96-113 / :151-168
            std::string cmd = "lastz " + cfg.data_folder + "ref.2bit[nameparse=darkspace][multiple][subset=ref_block" +
                              std::to_string(r_block_index) + ".name] " + cfg.data_folder +
                              "query.2bit[nameparse=darkspace][subset=query_block" + std::to_string(q_block_index) +
                              ".name] --format=" + cfg.output_format + " --ydrop=" + std::to_string(cfg.ydrop) +
                              " --gappedthresh=" + std::to_string(cfg.gappedthresh) + " --strand=" + (rev ? "minus" : "plus");
            if (cfg.ambiguous != "") cmd += " --ambiguous=" + cfg.ambiguous;
            if (cfg.notrivial) cmd += " --notrivial";
            if (cfg.scoring_file != "") cmd += " --scoring=" + cfg.scoring_file;
            cmd += " --segments=" + seg_name + " --output=" + base + "." + cfg.output_format + " 2> " + base + ".err";
            std::lock_guard<std::mutex> lk(io_lock);
            printf("%s\n", cmd.c_str());
        }
    }
}

static void usage();
static void usage_lift() {
    fprintf(stderr,
            "  --gpu_lift=FILE[,num/den] (with --gpu_net_subset: FILE is a BED file: target record, 0-based start, end, the rest of the line kept\n"
            "      as it is.  Next to each .net.chains file a .lifted.bed file: every line whose interval lies inside the file's target block and\n"
            "      of which exactly one sub-chain holds at least num/den of the bases (default 95/100), as query record, start, end within the\n"
            "      record (of the reverse complement in a .minus file), the rest of the line and the strand of the file, in input order; and an\n"
            "      .unlifted.bed file: every other such line after a line #Deleted (no sub-chain holds a base of it), #Partially deleted (none\n"
            "      holds enough) or #Duplicated (several do).  Merging the files of several blocks or strands is the caller's)\n");
}
static void usage() {
    fprintf(stderr,
            "Usage: segalign_host target.fa query.fa [data_folder/] [options]\n"
            "  --strand=plus|minus|both  --seed=12of19|14of22|<pattern of 0/1>  --step=N  --notransition\n"
            "  --xdrop=N --hspthresh=N --noentropy --nogapped --ydrop=N --gappedthresh=N --notrivial --format=F\n"
            "  --ambiguous=x|n|iupac[,reward,penalty] --scoring=FILE\n"
            "  --wga_chunk=N --lastz_interval=N --seq_block_size=N --num_gpu=N --num_threads=N --outdir=DIR\n"
            "  --host-seeding (build seed vectors on the host like src/seeder.cpp) --debug\n"
            "  --gpu_gapped [--gap=O,E] (gapped y-drop extension on the GPU: a .gapped file next to each .segments file)\n"
            "  --gpu_maf (with --gpu_gapped: the alignments of each .gapped file as a .maf file in LASTZ's maf- layout)\n"
            "  --gpu_skip_covered (with --gpu_gapped: extend anchors best first and skip those on earlier alignments)\n"
            "  --gpu_max_extent=N (with --gpu_gapped: bases one piece of an alignment side may span; default 65536)\n"
            "  --gpu_pieces=N (with --gpu_gapped: continue an alignment side that ends at the extent cap, up to N pieces; default 1)\n"
            "  --gpu_chain[=diag,anti] (a .chain file next to each .segments file: the best collinear chain of every target record x query\n"
            "      record pair, with penalties per diagonal and antidiagonal step, default 0,0; --gpu_gapped then extends the chains' HSPs only)\n"
            "  --gpu_chain_gap=N (with --gpu_chain: largest gap between consecutive chain members in either sequence; default 0, unlimited)\n"
            "      a .segments file may hold at most 4194304 HSPs with --gpu_chain\n"
            "  --gpu_chain_all[=diag,anti] (instead of --gpu_chain: a .chains file next to each .segments file with ALL collinear chains of\n"
            "      every pair, peeled best first, each under a line '#chain k group=g score=s members=m joined=0|1'; takes --gpu_chain_gap and\n"
            "      the same limit; --gpu_gapped then extends the HSPs of the chains kept)\n"
            "  --gpu_chain_min=N (with --gpu_chain_all: chains that score less than N are not kept; default 0)\n"
            "  --gpu_chain_costs=loose|medium|FILE (with --gpu_chain or --gpu_chain_all: a link also pays a piecewise-linear gap cost, in the\n"
            "      spirit of axtChain -linearGap: its two preset tables, or a FILE in its layout with at most 16 break points: lines\n"
            "      'tableSize N', 'smallSize N' (ignored), 'position ...', 'qGap ...', 'tGap ...', 'bothGap ...')\n"
            "  --gpu_chain_overlap[=N] (with --gpu_chain or --gpu_chain_all: two chained HSPs may share up to N bases, default 64, at most 4096 and\n"
            "      less than half of the shorter, on either sequence, as HSPs on the two sides of an indel do; every overlap is then cut where the\n"
            "      two together score best, so the .chain / .chains files hold the trimmed members with their exact scores and the exact chain\n"
            "      scores, and every later stage of the run gets those)\n"
            "  --gpu_chain_fill[=thresh[,xdrop]] (with --gpu_chain or --gpu_chain_all: every diagonal of the space between consecutive members of a\n"
            "      chain is scanned for ungapped HSPs the seeds missed, default 3000,910, and the best collinear chain of them is spliced in; a\n"
            "      .filled.chain / .filled.chains file next to each .chain / .chains file, and every later stage works on the filled chains)\n"
            "  --gpu_chain_fill_side=N (with --gpu_chain_fill: a space with a side above N is not scanned; default 32768, at most 1048576)\n"
            "  --gpu_stitch[=max_link] (with --gpu_chain or --gpu_chain_all: a .stitched.maf file next to each .chain / .chains file with every\n"
            "      chain as one alignment through all its members, the stretch between two members aligned globally with --gap=O,E; a chain\n"
            "      is cut where a side of that stretch exceeds max_link (default and at most 2048) or holds a record boundary)\n"
            "  --gpu_diff[=base] (with --gpu_maf or --gpu_stitch: a .diff file next to each .maf, .stitched.maf and .net.maf file: per alignment a\n"
            "      line '#a <k> <tname> <tstart> <qname> <+|-> <qstart> columns= matches= transitions= transversions= others= ins=<runs>/<bases>\n"
            "      del=<runs>/<bases> events= identity=<matches>/<columns>', then per difference '<sub|other|ins|del> <tname> <tstart> <qname>\n"
            "      <+|-> <qstart> <length> <tbase> <qbase>', starts 0-based within the record, '-' for the base a gap lacks; =base: one line per\n"
            "      substituted base instead of one per run)\n"
            "  --gpu_stitch_min=N (with --gpu_stitch: a chain is also cut at a stretch whose alignment scores less than N)\n"
            "  --gpu_net[=min_space] (with --gpu_chain_all: a .net file next to each .chains file: the kept chains of every target record laid\n"
            "      on the target best first, each filling what is still open, the gaps inside a fill open to lower chains one level down; a\n"
            "      line 'net <target record> <length>' per record, then per fill, indented by its depth, 'fill <tstart> <tsize> <qname> <+|->\n"
            "      <qstart> <qsize> chain=<k> score=<s> ali=<n>'; open stretches shorter than min_space, default 1, are not searched)\n"
            "  --gpu_net_fill=N (with --gpu_net: a chain fills an open stretch only with at least N bases in it; default 1)\n"
            "  --gpu_net_subset (with --gpu_net: a .net.chains file next to each .net file: every fill's part of its chain as a chain of its\n"
            "      own, cut where a lower chain fills one of its gaps, clipped members rescored, under the penalties of --gpu_chain_all and\n"
            "      --gpu_chain_costs; per sub-chain a line `#chain k fill=F run=R score=S` with its target and query extents, then its members\n"
            "      as .segments lines; with --gpu_stitch also a .net.maf file: those sub-chains stitched, in the .stitched.maf layout)\n"
            "  --gpu_net_class (with --gpu_net: a .net.class file next to each .net file: its lines with ' type=<top|syn|inv|nonSyn> qover=N\n"
            "      qfar=N qdup=N' appended to every fill line: a fill without a parent is top; one on another query record than its parent is\n"
            "      nonSyn; otherwise syn, with the bases its query extent shares with its parent's (qover) or the distance between the two\n"
            "      (qfar); qdup counts its query bases that another fill of the file claims too.  A file holds one strand, so inv, a fill on\n"
            "      the other strand than its parent, cannot occur here: it is reachable through sa_net_classify only)\n"
            "  --gpu_net_syn=min_score,min_top_score,min_size,min_ali,max_far (implies --gpu_net_class: a fill is kept if it scores at least\n"
            "      min_score, spans at least min_size target bases, holds at least min_ali aligned bases and, as a top fill, scores at least\n"
            "      min_top_score, as a syn fill lies at most max_far from its parent on the query; a nonSyn fill is dropped, and a dropped\n"
            "      fill takes the fills inside its gaps with it.  The .net.class file then holds the kept fills only, and --gpu_net_subset\n"
            "      works on them: .net.chains and .net.maf are the syntenic net's alignments)\n");
    usage_lift();
}

// A gap-cost table in axtChain's linearGap layout (see usage).  The file's form is checked here; the values are checked again by the
// chaining entry, so they are checked here too, to fail before any GPU work.  Returns false with a message in err.
static bool read_linear_gap(const std::string& path, sa_chain_gap_costs& out, std::string& err) {
    FILE* f = fopen(path.c_str(), "r");
    if (!f) { err = "cannot open it"; return false; }
    memset(&out, 0, sizeof(out));
    const char* names[6] = {"tableSize", "smallSize", "position", "qGap", "tGap", "bothGap"};
    std::vector<long long> vals[6];
    bool seen[6] = {false, false, false, false, false, false};
    char line[4096];
    while (fgets(line, sizeof(line), f)) {
        char* tok = strtok(line, " \t\r\n");
        if (!tok || tok[0] == '#') continue;
        int w = -1;
        for (int k = 0; k < 6; k++) if (!strcmp(tok, names[k])) w = k;
        if (w < 0 || seen[w]) { err = std::string("unknown or repeated line ") + tok; fclose(f); return false; }
        seen[w] = true;
        while ((tok = strtok(nullptr, " \t\r\n"))) {
            char* endp = nullptr;
            const long long x = strtoll(tok, &endp, 10);
            if (endp == tok || *endp) { err = std::string(names[w]) + ": " + tok + " is not an integer"; fclose(f); return false; }
            vals[w].push_back(x);
        }
    }
    fclose(f);
    for (int k = 0; k < 6; k++) if (k != 1 && !seen[k]) { err = std::string("no ") + names[k] + " line"; return false; }
    if (vals[0].size() != 1 || (seen[1] && vals[1].size() != 1)) { err = "tableSize and smallSize take one value"; return false; }
    const long long n = vals[0][0];
    if (n < 1 || n > SA_CHAIN_GAP_POINTS) { err = "tableSize is not in 1 .. 16"; return false; }
    for (int k = 2; k < 6; k++) if ((long long)vals[k].size() != n) { err = std::string(names[k]) + " does not have tableSize values"; return false; }
    out.n = (uint32_t)n;
    int64_t* cost[3] = {out.q_gap, out.t_gap, out.both_gap};
    for (long long k = 0; k < n; k++) {
        if (vals[2][k] < 1 || vals[2][k] > 0xffffffffll || (k > 0 && vals[2][k] <= vals[2][k - 1])) { err = "position must ascend strictly from at least 1"; return false; }
        out.pos[k] = (uint32_t)vals[2][k];
        for (int a = 0; a < 3; a++) {
            const long long c = vals[3 + a][k];
            if (c < 0 || c > (1ll << 40) || (k > 0 && c < vals[3 + a][k - 1])) { err = std::string(names[3 + a]) + " must be non-decreasing within 0 .. 2^40"; return false; }
            if (k > 0 && ((c - vals[3 + a][k - 1]) << 16) / (vals[2][k] - vals[2][k - 1]) >= (1ll << 27)) { err = std::string(names[3 + a]) + " rises by 2048 or more per base"; return false; }
            cost[a][k] = c;
        }
    }
    return true;
}

int main(int argc, char** argv) {
    setenv("GPU_MAX_HW_QUEUES", "8", 0);  // the host's own choice, before the first HIP call: one hardware queue per engine slot
    std::vector<std::string> pos;
    for (int i = 1; i < argc; i++) {
        std::string v;
        const char* a = argv[i];
        if (a[0] != '-') pos.push_back(a);
        else if (!strcmp(a, "--help")) { usage(); return 0; }
        else if (opt(a, "--strand", v)) cfg.strand = v;
        else if (opt(a, "--seed", v)) cfg.seed_shape = v;
        else if (opt(a, "--step", v)) cfg.step = (uint32_t)atoi(v.c_str());
        else if (!strcmp(a, "--notransition")) cfg.transition = false;
        else if (opt(a, "--xdrop", v)) cfg.xdrop = atoi(v.c_str());
        else if (opt(a, "--hspthresh", v)) cfg.hspthresh = atoi(v.c_str());
        else if (!strcmp(a, "--noentropy")) cfg.noentropy = true;
        else if (!strcmp(a, "--nogapped")) cfg.gapped = false;
        else if (opt(a, "--ydrop", v)) cfg.ydrop = atoi(v.c_str());
        else if (opt(a, "--gappedthresh", v)) cfg.gappedthresh = atoi(v.c_str());
        else if (!strcmp(a, "--notrivial")) cfg.notrivial = true;
        else if (opt(a, "--format", v)) cfg.output_format = v;
        else if (opt(a, "--ambiguous", v)) cfg.ambiguous = v;
        else if (opt(a, "--scoring", v)) cfg.scoring_file = v;
        else if (opt(a, "--wga_chunk", v)) cfg.wga_chunk = (uint32_t)atol(v.c_str());
        else if (opt(a, "--lastz_interval", v)) cfg.lastz_interval = (uint32_t)atol(v.c_str());
        else if (opt(a, "--seq_block_size", v)) cfg.seq_block_size = (uint32_t)atol(v.c_str());
        else if (opt(a, "--num_gpu", v)) cfg.num_gpu = atoi(v.c_str());
        else if (opt(a, "--num_threads", v)) cfg.num_threads = atoi(v.c_str());
        else if (opt(a, "--outdir", v)) cfg.outdir = v;
        else if (!strcmp(a, "--host-seeding")) cfg.host_seeding = true;
        else if (!strcmp(a, "--debug")) cfg.debug = true;
        else if (!strcmp(a, "--gpu_gapped")) cfg.gpu_gapped = true;
        else if (!strcmp(a, "--gpu_maf")) cfg.gpu_maf = true;
        else if (!strcmp(a, "--gpu_skip_covered")) cfg.gpu_skip_covered = true;
        else if (opt(a, "--gpu_max_extent", v)) cfg.gpu_max_extent = (uint32_t)atol(v.c_str());
        else if (opt(a, "--gpu_pieces", v)) {
            cfg.gpu_pieces = atoi(v.c_str());
            if (cfg.gpu_pieces < 1 || cfg.gpu_pieces > 1024) { fprintf(stderr, "bad --gpu_pieces=%s (1 .. 1024)\n", v.c_str()); return 1; }
        }
        else if (!strcmp(a, "--gpu_chain")) cfg.gpu_chain = true;
        else if (opt(a, "--gpu_chain", v)) {
            cfg.gpu_chain = true;
            char tail;
            if (sscanf(v.c_str(), "%d,%d%c", &cfg.chain_diag, &cfg.chain_anti, &tail) != 2 || cfg.chain_diag < 0 || cfg.chain_diag > (1 << 20) ||
                cfg.chain_anti < 0 || cfg.chain_anti > (1 << 20)) { fprintf(stderr, "bad --gpu_chain=%s (diag,anti; each 0 .. %d)\n", v.c_str(), 1 << 20); return 1; }
        }
        else if (!strcmp(a, "--gpu_chain_all")) cfg.gpu_chain_all = true;
        else if (opt(a, "--gpu_chain_all", v)) {
            cfg.gpu_chain_all = true;
            char tail;
            if (sscanf(v.c_str(), "%d,%d%c", &cfg.chain_diag, &cfg.chain_anti, &tail) != 2 || cfg.chain_diag < 0 || cfg.chain_diag > (1 << 20) ||
                cfg.chain_anti < 0 || cfg.chain_anti > (1 << 20)) { fprintf(stderr, "bad --gpu_chain_all=%s (diag,anti; each 0 .. %d)\n", v.c_str(), 1 << 20); return 1; }
        }
        else if (opt(a, "--gpu_chain_min", v)) {
            char* endp = nullptr;
            cfg.chain_min = strtoll(v.c_str(), &endp, 10);
            if (endp == v.c_str() || *endp) { fprintf(stderr, "bad --gpu_chain_min=%s (an integer)\n", v.c_str()); return 1; }
            cfg.chain_min_set = true;
        }
        else if (opt(a, "--gpu_chain_gap", v)) {
            char* endp = nullptr;
            const long long gap = strtoll(v.c_str(), &endp, 10);
            if (endp == v.c_str() || *endp || gap < 0 || gap > 0xffffffffll) { fprintf(stderr, "bad --gpu_chain_gap=%s (0 .. 4294967295; 0: unlimited)\n", v.c_str()); return 1; }
            cfg.chain_gap = (uint32_t)gap;
        }
        else if (!strcmp(a, "--gpu_chain_overlap")) cfg.chain_overlap = 64;
        else if (opt(a, "--gpu_chain_overlap", v)) {
            char* endp = nullptr;
            const long long n = strtoll(v.c_str(), &endp, 10);
            if (endp == v.c_str() || *endp || n < 1 || n > SA_CHAIN_MAX_OVERLAP) { fprintf(stderr, "bad --gpu_chain_overlap=%s (1 .. %d)\n", v.c_str(), SA_CHAIN_MAX_OVERLAP); return 1; }
            cfg.chain_overlap = (uint32_t)n;
        }
        else if (!strcmp(a, "--gpu_chain_fill")) cfg.chain_fill = true;
        else if (opt(a, "--gpu_chain_fill", v)) {
            char* endp = nullptr;
            const long long th = strtoll(v.c_str(), &endp, 10);
            long long xd = cfg.fill_xdrop;
            bool ok = endp != v.c_str() && (*endp == 0 || *endp == ',') && th >= 1 && th <= INT32_MAX;
            if (ok && *endp == ',') {
                const char* x = endp + 1;
                xd = strtoll(x, &endp, 10);
                ok = endp != x && *endp == 0 && xd >= 0 && xd <= INT32_MAX;
            }
            if (!ok) { fprintf(stderr, "bad --gpu_chain_fill=%s (thresh[,xdrop]; thresh at least 1, xdrop at least 0)\n", v.c_str()); return 1; }
            cfg.chain_fill = true;
            cfg.fill_thresh = (int)th;
            cfg.fill_xdrop = (int)xd;
        }
        else if (opt(a, "--gpu_chain_fill_side", v)) {
            char* endp = nullptr;
            const long long n = strtoll(v.c_str(), &endp, 10);
            if (endp == v.c_str() || *endp || n < 1 || n > (1 << 20)) { fprintf(stderr, "bad --gpu_chain_fill_side=%s (1 .. %d)\n", v.c_str(), 1 << 20); return 1; }
            cfg.fill_side = (uint32_t)n;
            cfg.fill_side_set = true;
        }
        else if (opt(a, "--gpu_chain_costs", v)) {
            std::string err;
            if (sa_chain_gap_preset(v.c_str(), &cfg.chain_costs) != 0 && !read_linear_gap(v, cfg.chain_costs, err)) {
                fprintf(stderr, "bad --gpu_chain_costs=%s (loose, medium or a linearGap file): %s\n", v.c_str(), err.c_str());
                return 1;
            }
            cfg.chain_costs_set = true;
        }
        else if (!strcmp(a, "--gpu_stitch")) cfg.gpu_stitch = true;
        else if (opt(a, "--gpu_stitch", v)) {
            char* endp = nullptr;
            const long long ml = strtoll(v.c_str(), &endp, 10);
            if (endp == v.c_str() || *endp || ml < 1 || ml > 2048) { fprintf(stderr, "bad --gpu_stitch=%s (max_link: 1 .. 2048)\n", v.c_str()); return 1; }
            cfg.gpu_stitch = true;
            cfg.stitch_max_link = (uint32_t)ml;
        }
        else if (!strcmp(a, "--gpu_diff")) cfg.gpu_diff = true;
        else if (opt(a, "--gpu_diff", v)) {
            if (v != "base") { fprintf(stderr, "bad --gpu_diff=%s (base, or no value)\n", v.c_str()); return 1; }
            cfg.gpu_diff = cfg.diff_per_base = true;
        }
        else if (opt(a, "--gpu_stitch_min", v)) {
            char* endp = nullptr;
            const long long ms = strtoll(v.c_str(), &endp, 10);
            if (endp == v.c_str() || *endp || ms < INT32_MIN || ms > INT32_MAX) { fprintf(stderr, "bad --gpu_stitch_min=%s (a 32-bit integer)\n", v.c_str()); return 1; }
            cfg.stitch_min = (int)ms;
            cfg.stitch_min_set = true;
        }
        else if (!strcmp(a, "--gpu_net")) cfg.gpu_net = true;
        else if (opt(a, "--gpu_net", v)) {
            char* endp = nullptr;
            const long long ms = strtoll(v.c_str(), &endp, 10);
            if (endp == v.c_str() || *endp || ms < 1 || ms > (1ll << 31)) { fprintf(stderr, "bad --gpu_net=%s (min_space: 1 .. 2147483648)\n", v.c_str()); return 1; }
            cfg.gpu_net = true;
            cfg.net_space = (uint32_t)ms;
        }
        else if (!strcmp(a, "--gpu_net_subset")) cfg.gpu_net_subset = true;
        else if (!strcmp(a, "--gpu_net_class")) cfg.gpu_net_class = true;
        else if (opt(a, "--gpu_lift", v)) {
            cfg.lift_bed = v;
            const size_t comma = v.rfind(',');
            unsigned long long num = 0, den = 0;
            char tail = 0;
            if (comma != std::string::npos && sscanf(v.c_str() + comma + 1, "%llu/%llu%c", &num, &den, &tail) == 2) {
                if (den < 1 || den > (1ull << 20) || num > den) {
                    fprintf(stderr, "bad --gpu_lift=%s (num/den with 1 <= den <= 1048576 and num <= den)\n", v.c_str());
                    return 1;
                }
                cfg.lift_p = {(uint32_t)num, (uint32_t)den};
                cfg.lift_bed = v.substr(0, comma);
            }
            if (cfg.lift_bed.empty()) { fprintf(stderr, "bad --gpu_lift=%s (a BED file)\n", v.c_str()); return 1; }
            cfg.gpu_lift = true;
        }
        else if (opt(a, "--gpu_net_syn", v)) {
            long long t[5];
            char tail = 0;
            const bool ok = sscanf(v.c_str(), "%lld,%lld,%lld,%lld,%lld%c", &t[0], &t[1], &t[2], &t[3], &t[4], &tail) == 5;
            if (!ok || t[2] < 0 || t[2] > (1ll << 31) || t[3] < 0 || t[3] > (1ll << 31) || t[4] < 0 || t[4] > (1ll << 31)) {
                fprintf(stderr, "bad --gpu_net_syn=%s (min_score,min_top_score,min_size,min_ali,max_far; the last three 0 .. 2147483648)\n", v.c_str());
                return 1;
            }
            cfg.net_syn_p = {t[0], t[1], (uint32_t)t[2], (uint32_t)t[3], (uint32_t)t[4], 0};
            cfg.net_syn = cfg.gpu_net_class = true;
        }
        else if (opt(a, "--gpu_net_fill", v)) {
            char* endp = nullptr;
            const long long mf = strtoll(v.c_str(), &endp, 10);
            if (endp == v.c_str() || *endp || mf < 1 || mf > (1ll << 31)) { fprintf(stderr, "bad --gpu_net_fill=%s (1 .. 2147483648)\n", v.c_str()); return 1; }
            cfg.net_fill = (uint32_t)mf;
            cfg.net_fill_set = true;
        }
        else if (opt(a, "--gap", v)) {
            if (sscanf(v.c_str(), "%d,%d", &cfg.gap_open, &cfg.gap_extend) != 2) { fprintf(stderr, "bad --gap=%s\n", v.c_str()); return 1; }
        }
        else { fprintf(stderr, "unknown option %s\n", a); usage(); return 1; }
    }
    if (pos.size() < 2) {
        fprintf(stderr, "You must specify a target file and a query file\n");
        usage();
        return 1;
    }
    if (cfg.gpu_chain && cfg.gpu_chain_all) { fprintf(stderr, "--gpu_chain and --gpu_chain_all exclude each other\n"); return 1; }
    if (cfg.chain_min_set && !cfg.gpu_chain_all) { fprintf(stderr, "--gpu_chain_min needs --gpu_chain_all\n"); return 1; }
    if (cfg.chain_costs_set && !cfg.gpu_chain && !cfg.gpu_chain_all) { fprintf(stderr, "--gpu_chain_costs needs --gpu_chain or --gpu_chain_all\n"); return 1; }
    if (cfg.chain_overlap && !cfg.gpu_chain && !cfg.gpu_chain_all) { fprintf(stderr, "--gpu_chain_overlap needs --gpu_chain or --gpu_chain_all\n"); return 1; }
    if (cfg.chain_fill && !cfg.gpu_chain && !cfg.gpu_chain_all) { fprintf(stderr, "--gpu_chain_fill needs --gpu_chain or --gpu_chain_all\n"); return 1; }
    if (cfg.fill_side_set && !cfg.chain_fill) { fprintf(stderr, "--gpu_chain_fill_side needs --gpu_chain_fill\n"); return 1; }
    if (cfg.gpu_stitch && !cfg.gpu_chain && !cfg.gpu_chain_all) { fprintf(stderr, "--gpu_stitch needs --gpu_chain or --gpu_chain_all\n"); return 1; }
    if (cfg.gpu_diff && !cfg.gpu_maf && !cfg.gpu_stitch) { fprintf(stderr, "--gpu_diff needs --gpu_maf or --gpu_stitch\n"); return 1; }
    if (cfg.stitch_min_set && !cfg.gpu_stitch) { fprintf(stderr, "--gpu_stitch_min needs --gpu_stitch\n"); return 1; }
    if (cfg.gpu_net && !cfg.gpu_chain_all) { fprintf(stderr, "--gpu_net needs --gpu_chain_all\n"); return 1; }
    if (cfg.gpu_net_subset && !cfg.gpu_net) { fprintf(stderr, "--gpu_net_subset needs --gpu_net and --gpu_chain_all\n"); return 1; }
    if (cfg.gpu_net_class && !cfg.gpu_net) { fprintf(stderr, "%s needs --gpu_net and --gpu_chain_all\n", cfg.net_syn ? "--gpu_net_syn" : "--gpu_net_class"); return 1; }
    if (cfg.gpu_lift && !cfg.gpu_net_subset) { fprintf(stderr, "--gpu_lift needs --gpu_net_subset, --gpu_net and --gpu_chain_all\n"); return 1; }
    if (cfg.net_fill_set && !cfg.gpu_net) { fprintf(stderr, "--gpu_net_fill needs --gpu_net and --gpu_chain_all\n"); return 1; }
    cfg.target = pos[0];
    cfg.query = pos[1];
    if (pos.size() > 2) cfg.data_folder = pos[2];
    if (cfg.gappedthresh < 0) cfg.gappedthresh = cfg.hspthresh;  // src/main.cpp:182-183
    // seed shape, src/main.cpp:160-180
    if (cfg.seed_shape == "12of19") cfg.shape = "TTT0T00TT00T0T0TTTT";
    else if (cfg.seed_shape == "14of22") cfg.shape = "TTT0T0TT00TT00T0T0TTTT";
    else { cfg.shape = cfg.seed_shape; for (auto& c : cfg.shape) c = (c == '1') ? 'T' : '0'; }
    cfg.seed_size = (uint32_t)cfg.shape.size();
    shape_weight = 0;
    for (size_t i = 0; i < cfg.shape.size(); i++)
        if (cfg.shape[i] == '1' || cfg.shape[i] == 'T') { transition_pos[shape_weight] = cfg.shape[i] == 'T'; shape_pos[shape_weight++] = (int)i; }
    cfg.kmer_size = shape_weight;
    if (cfg.num_threads <= 0) cfg.num_threads = std::max(2u, std::thread::hardware_concurrency());
    cfg.num_threads = std::min(cfg.num_threads, 64);

    int sub_mat[64];
    build_sub_mat(sub_mat, cfg.ambiguous, cfg.scoring_file, cfg.xdrop);
    fprintf(stderr, "Using %d threads\n", cfg.num_threads);
    cfg.num_gpu = sa_initialize_interface(cfg.num_gpu);                                                        // main.cpp:297
    sa_generate_shape_pos(cfg.shape.c_str());                                                                 // main.cpp:180
    {   // one engine slot per seeder thread, up to four calls in flight per device (more only queue behind the filter kernels)
        char slots[16];
        snprintf(slots, sizeof(slots), "%d", std::max(2, std::min(4, cfg.num_threads)));
        setenv("SEGALIGN_AMD_SLOTS", slots, 0);
    }
    if (cfg.gpu_pieces > 0) sa_set_option("gapped_pieces", cfg.gpu_pieces);
    sa_initialize_processor(cfg.transition, cfg.wga_chunk, cfg.seed_size, sub_mat, cfg.xdrop, cfg.hspthresh, cfg.noentropy);  // :298

    auto t0 = std::chrono::steady_clock::now();
    fprintf(stderr, "\nReading query file ...\n");
    load_set(cfg.query, Q, true, "query");
    fprintf(stderr, "\nReading target file ...\n");
    load_set(cfg.target, R, false, "ref");
    if (cfg.gpu_lift) load_bed(cfg.lift_bed);
    auto t1 = std::chrono::steady_clock::now();
    fprintf(stderr, "\nStart alignment ...\n");

    double table_ms = 0;
    uint64_t query_bases_done = 0;
    for (size_t rb = 0; rb < R.block_len.size(); rb++) {
        fprintf(stderr, "\nSending reference block %zu ...\n", rb);
        if (rb > 0) sa_clear_ref();                                                                            // :613
        sa_send_ref_write_request(R.buf.data(), R.block_start[rb], R.block_len[rb]);                           // :615
        auto ta = std::chrono::steady_clock::now();
        sa_generate_seed_pos_table(R.buf.data(), R.block_start[rb], R.block_len[rb], cfg.step, (int)cfg.seed_size, cfg.kmer_size);  // :621
        table_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ta).count();

        const size_t nqb = Q.block_len.size();
        std::thread uploader;
        auto upload = [&](size_t qb) {  // :659-661 / :680-681
            uint32_t buffer = (uint32_t)(qb % SA_BUFFER_DEPTH);
            if (rb > 0 || qb >= SA_BUFFER_DEPTH) sa_clear_query(buffer);
            sa_send_query_write_request(Q.buf.data(), Q.block_start[qb], Q.block_len[qb], buffer);
        };
        if (nqb > 0) upload(0);
        for (size_t qb = 0; qb < nqb; qb++) {
            if (uploader.joinable()) uploader.join();
            if (qb + 1 < nqb) uploader = std::thread(upload, qb + 1);  // next block into the other device buffer while this one runs
            const uint32_t buffer = (uint32_t)(qb % SA_BUFFER_DEPTH);
            const std::vector<Interval>& ivs = q_intervals[qb];
            const uint32_t q_len = Q.block_len[qb] - cfg.seed_size;                                             // :708
            std::atomic<size_t> next(0);
            auto worker = [&]() {
                for (;;) {
                    size_t i = next.fetch_add(1);
                    if (i >= ivs.size()) return;
                    fprintf(stderr, "Query block %zu, interval %zu/%zu (%u:%u) with buffer %u\n", qb, i + 1, ivs.size(),
                            ivs[i].start, ivs[i].end, buffer);                                                   // seeder.cpp:45
                    Hsps h;
                    seed_interval(Q.block_start[qb], q_len, ivs[i], buffer, h);
                    print_segments((int)rb, (int)qb, R.block_start[rb], Q.block_start[qb], (uint32_t)i + 1, h, buffer);
                }
            };
            std::vector<std::thread> pool;
            int nt = (int)std::min<size_t>((size_t)cfg.num_threads, std::max<size_t>(ivs.size(), 1));
            for (int t = 0; t < nt; t++) pool.emplace_back(worker);
            for (auto& t : pool) t.join();
            query_bases_done += Q.block_len[qb];
        }
        if (uploader.joinable()) uploader.join();
    }
    auto t2 = std::chrono::steady_clock::now();
    sa_shutdown_processor();                                                                                   // :743
    if (cfg.debug) {  // src/main.cpp:617-629,745-752
        double load_s = std::chrono::duration<double>(t1 - t0).count(), run_s = std::chrono::duration<double>(t2 - t1).count();
        fprintf(stderr, "Time elapsed (loading sequences): %.3f sec\n", load_s);
        fprintf(stderr, "Time elapsed (seed position table create on GPU): %.1f msec\n", table_ms);
        fprintf(stderr, "Time elapsed (complete pipeline): %.3f sec  (%.4f Gbp of query x %zu target block(s) per sec)\n", run_s,
                query_bases_done / run_s / 1e9, R.block_len.size());
        fprintf(stderr, "#seed hits: %lu \n#HSPs: %lu \n", (unsigned long)g_num_seed_hits.load(), (unsigned long)g_num_hsps.load());
    }
    return 0;
}
