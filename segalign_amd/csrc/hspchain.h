// hspchain.h -- what hspchain.hip (the kernels) and api_hspchain.hip (sa_chain_hsps) share.  Contract: include/segalign_amd.h, DESIGN.md 15.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/segalign_amd.h"

namespace sa {

constexpr uint32_t HSPCHAIN_NONE = 0xFFFFFFFFu;  // pred of a node without predecessor
constexpr uint32_t HSPCHAIN_MAX_N = 1u << 22;

// The HSPs in canonical rank order (group, ref_start, query_start, len, input index), one array per field, and the DP's results.
struct HspChainArgs {
    const uint32_t *rs, *qs, *ln, *gr;  // ref_start, query_start, len (bases - 1), group
    const int32_t* sc;
    int64_t* f;
    uint32_t* pred;  // rank of the predecessor, or HSPCHAIN_NONE
    uint32_t n, tile;  // tile: a power of two, 64 .. 1024; tile b holds ranks [b tile, min(n, (b + 1) tile))
    int32_t diag_pen, anti_pen;
    uint32_t max_gap;
};

struct HspChainPartial {  // the best candidate one earlier tile offers a node: value > 0 and the lowest rank that reaches it, or (0, NONE)
    int64_t v;
    uint32_t rank, pad;
};

// What the overlap instances of the DP (hspovl.hip) know of a node beyond HspChainArgs, in rank order, both made by the
// weight kernel: w = floor(65536 max(score, 0) / bases), below 2^47, and lim = min(len >> 1, max_overlap), the largest overlap the node
// takes part in.  A separate struct, so that the kernel arguments of the plain instances stay what they were.
struct HspOvlNodes {
    const int64_t* w;
    const uint32_t* lim;
};

// ---- rank ----
// key[i] = query_start << 32 | len, idx[i] = i: the first (minor) stable sort.
void launch_hspchain_key_minor(const sa_segment_pair* hsps, uint32_t n, uint64_t* key, uint32_t* idx, hipStream_t s);
// key[p] = group << 32 | ref_start of HSP idx[p]: the second (major) stable sort.  group may be nullptr (all 0).
void launch_hspchain_key_major(const sa_segment_pair* hsps, const uint32_t* group, const uint32_t* idx, uint32_t n, uint64_t* key, hipStream_t s);
// The ranked field arrays from order[rank] = input index; head[r] = 1 where rank r starts a group, head[n] = 0.
void launch_hspchain_gather(const sa_segment_pair* hsps, const uint32_t* group, const uint32_t* order, uint32_t n, uint32_t* rs, uint32_t* qs,
                            uint32_t* ln, int32_t* sc, uint32_t* gr, uint32_t* head, hipStream_t s);
// first[b] = the first tile that holds a node of the group of tile b's first node.
void launch_hspchain_first(const uint32_t* gr, uint32_t n, uint32_t tile, uint32_t* first, hipStream_t s);

// ---- the DP, tile by tile in rank order ----
// image: the device image of a gap-cost table (hspcost.h: HSPCOST_WORDS words, 16-byte aligned), whose cost joins the penalty of every
// link, or nullptr for the linear penalty alone; same grid and same partials either way.
// Cross: workgroup k of b - c0 offers tile c = c0 + k to every node of tile b; partial[k * tile + t] for node b * tile + t.
void launch_hspchain_cross(const HspChainArgs& a, uint32_t b, uint32_t c0, HspChainPartial* partial, const uint32_t* image, hipStream_t s);
// Resolve: one workgroup reduces tile b's partials over c, settles the tile's own dependencies and writes its f and pred.
void launch_hspchain_resolve(const HspChainArgs& a, uint32_t b, uint32_t c0, const HspChainPartial* partial, const uint32_t* image, hipStream_t s);

// ---- the DP under an overlap allowance (hspovl.hip) ----
// w[r], lim[r] of HspOvlNodes for every rank r < n from a.ln and a.sc: one division per node.
void launch_hspovl_weight(const HspChainArgs& a, uint32_t max_overlap, int64_t* w, uint32_t* lim, hipStream_t s);
// launch_hspchain_cross and launch_hspchain_resolve under the relation, gaps and charge of sa_chain_hsps_ovl: same grids, same partials.
void launch_hspovl_cross(const HspChainArgs& a, const HspOvlNodes& o, uint32_t b, uint32_t c0, HspChainPartial* partial, const uint32_t* image,
                         hipStream_t s);
void launch_hspovl_resolve(const HspChainArgs& a, const HspOvlNodes& o, uint32_t b, uint32_t c0, const HspChainPartial* partial,
                           const uint32_t* image, hipStream_t s);

// ---- finish ----
// gstart[g] = first rank of the g-th group, from the head flags and their exclusive scan.
void launch_hspchain_group_starts(const uint32_t* head, const uint64_t* gidx, uint32_t n, uint32_t* gstart, hipStream_t s);
// One wave per group: gend[g] = the rank with the group's largest f (lowest rank among equals), glen[g] = members of the pred walk
// from there, or 0 when that f is below min_score; glen[groups] = 0.
void launch_hspchain_ends(const HspChainArgs& a, const uint32_t* gstart, uint32_t groups, int64_t min_score, uint32_t* gend, uint32_t* glen,
                          hipStream_t s);
// One thread per group writes its chain's members in rank order at goff[g].
void launch_hspchain_members(const HspChainArgs& a, const uint32_t* order, const uint32_t* gend, const uint32_t* glen, const uint64_t* goff,
                             uint32_t groups, sa_chain_member* out, hipStream_t s);
// nodes[order[r]] = {f[r], input index of pred[r] or -1}.
void launch_hspchain_nodes(const HspChainArgs& a, const uint32_t* order, sa_chain_node* nodes, hipStream_t s);

}  // namespace sa
