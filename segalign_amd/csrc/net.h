// net.h -- what net.hip (the kernels) and api_net.hip (sa_net_chains) share.  Contract: include/segalign_amd.h, DESIGN.md 19.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/segalign_amd.h"

namespace sa {

constexpr uint32_t NET_NONE = 0xFFFFFFFFu;
constexpr uint32_t NET_TOP = 1u << 31;             // the root space is [0, NET_TOP)
constexpr uint32_t NET_MAX_CHAINS = 1u << 22;
constexpr uint32_t NET_MAX_BLOCKS = 1u << 26;

// An open space that a round searches: [a, b) and the priority positions [from, hi) that may still fill it.
struct NetSpace {
    uint32_t a, b;
    uint32_t from, hi;
    int32_t parent;  // fill that opened it (index in emission order), or -1
    uint32_t depth;
};

// What the search leaves per space: the filler's priority position (NET_NONE: none), its first and last clipped block and their bases.
struct NetHit {
    uint32_t pos, i, j, ali;
};

// Every per-chain array is indexed by priority position unless its comment names another index.
struct NetArgs {
    const uint32_t *bs, *be;    // [blocks] the blocks, input order
    const uint32_t* first;      // [n + 1] by chain
    const int64_t* score;       // by chain
    const uint32_t* group;      // by chain, or nullptr
    uint32_t n, blocks;
    uint32_t min_space, min_fill;
    uint64_t *key_a, *key_b;    // [n] sort keys, in and out
    uint32_t *idx_a, *idx_b;    // [n] sort values, in and out
    uint32_t* byprio;           // position -> chain
    uint32_t *hull_s, *hull_e;  // [first start, last end), (0, 0) for an empty chain
    uint32_t* head;             // [n + 1] 1 where a group's range of positions starts; head[n] = 0
    uint64_t* gidx;             // [n + 1] exclusive scan of head; gidx[n] = groups
    uint32_t* gstart;           // [groups + 1] group -> its first position; gstart[groups] = n
    uint32_t* len;              // [blocks] block lengths
    uint64_t* pre;              // [blocks + 1] their exclusive prefix sums
};

// One round over S spaces.  cnt holds 2 S entries: [0, S) the searched children of a space, [S, 2 S) 1 for a space that is filled; off
// (2 S + 1 entries) is cnt's exclusive scan, so off[S] = children and off[2 S] - off[S] = fills of the round.
struct NetRound {
    const NetSpace* spaces;
    uint32_t S;
    NetHit* hit;
    uint32_t* cnt;
    uint64_t* off;
    NetSpace* next;       // the next round's spaces
    sa_net_fill* fills;   // all fills in emission order
    uint32_t fill_base;   // fills before this round
};

// len[k] = be[k] - bs[k].
void launch_net_block_len(const NetArgs& a, hipStream_t s);
// key_a[c] = score[c] ordered descending, idx_a[c] = c: the minor sort.
void launch_net_key_minor(const NetArgs& a, hipStream_t s);
// key_a[p] = group of chain idx[p] (0 without groups): the major sort.
void launch_net_key_major(const NetArgs& a, const uint32_t* idx, hipStream_t s);
// From byprio: hull_s, hull_e and head.
void launch_net_gather(const NetArgs& a, hipStream_t s);
// gstart from head and gidx.
void launch_net_group_starts(const NetArgs& a, hipStream_t s);
// The root space of every group.
void launch_net_roots(const NetArgs& a, uint32_t groups, NetSpace* spaces, hipStream_t s);
// One wavefront per space: the first position in [from, hi) whose chain holds at least min_fill bases in [a, b).
void launch_net_search(const NetArgs& a, const NetRound& r, hipStream_t s);
// One wavefront per space: cnt[k] = its remainders and gaps of at least min_space, cnt[S + k] = it is filled.
void launch_net_count(const NetArgs& a, const NetRound& r, hipStream_t s);
// One wavefront per space: its fill, and its searched children into next.
void launch_net_emit(const NetArgs& a, const NetRound& r, hipStream_t s);
// key[f] = group << 32 | start, idx[f] = f over F fills.
void launch_net_fill_key(const sa_net_fill* fills, uint32_t F, uint64_t* key, uint32_t* idx, hipStream_t s);
// inv[order[k]] = k.
void launch_net_inverse(const uint32_t* order, uint32_t F, uint32_t* inv, hipStream_t s);
// out[k] = fills[order[k]] with its parent mapped through inv.
void launch_net_finish(const sa_net_fill* fills, const uint32_t* order, const uint32_t* inv, uint32_t F, sa_net_fill* out, hipStream_t s);

}  // namespace sa
