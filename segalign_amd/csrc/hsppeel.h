// hsppeel.h -- what hsppeel.hip (the kernels) and api_hspchain.hip (sa_chain_hsps_all) share.  Contract: include/segalign_amd.h, DESIGN.md 16.
#pragma once
#include "hspchain.h"

namespace sa {

// Every array is indexed by rank (the DP's order) unless its comment names another index.  NONE is HSPCHAIN_NONE.
struct HspPeelArgs {
    const int64_t* f;       // the DP's f
    const uint32_t* pred;   // the DP's pred (rank or NONE)
    const uint32_t* gr;     // group
    const uint32_t* order;  // rank -> input index
    uint32_t n;
    int64_t min_score;
    uint64_t *key_a, *key_b;   // sort keys, in and out
    uint32_t *idx_a, *idx_b;   // sort values, in and out
    uint32_t* byprio;          // priority position -> rank (the inverse of prio)
    uint32_t* val;             // starts as prio[r]; after the rounds the smallest prio in r's subtree
    uint32_t *ptr_a, *ptr_b;   // the doubled pointers, double-buffered
    uint32_t* head;            // rank of the head of r's chain
    int64_t* cscore;           // at a head: its chain's score
    uint32_t* cjoin;           // at a head: the rank its chain was cut at, or NONE
    uint32_t* corder;          // chain position -> head rank: heads first, by (group, score descending, head rank)
    uint32_t* cpos;            // head rank -> chain position
    uint32_t* keep;            // [n + 1] by chain position: 1 for a chain with score >= min_score
    uint64_t* kidx;            // [n + 1] exclusive scan of keep: the index of a kept chain; kidx[n] = chains kept
    uint32_t* khead;           // kept chain -> head rank
    uint32_t* first;           // [n + 1] kept chain -> its first member's position; first[chains kept] = members kept
    uint64_t* tot;             // [3] chains kept, members kept, chains before min_score
    sa_chain_record* chains;
    sa_chain_all_member* members;
    uint32_t* chain_of;        // by input index
};

// key_a[r] = f[r] ordered descending (sign bit flipped, then complemented), idx_a[r] = r.
void launch_hsppeel_prio_key(const HspPeelArgs& a, hipStream_t s);
// From byprio (the sorted ranks): val[byprio[p]] = p.
void launch_hsppeel_init(const HspPeelArgs& a, hipStream_t s);
// One doubling round: atomicMin(&val[ptr[r]], val[r]) and ptr_next[r] = ptr[ptr[r]] for every r with a live ptr.
void launch_hsppeel_round(const HspPeelArgs& a, const uint32_t* ptr, uint32_t* ptr_next, hipStream_t s);
// head[r] = byprio[val[r]]; the tail of every chain writes the chain's score and join to the slot of its head.
void launch_hsppeel_tails(const HspPeelArgs& a, hipStream_t s);
// key_a[r] = chain score of head r ordered descending (all ones where r is no head), idx_a[r] = r: the minor sort of the chains.
void launch_hsppeel_chain_key_minor(const HspPeelArgs& a, hipStream_t s);
// key_a[p] = (idx[p] is no head) << 32 | group of idx[p]: the major sort of the chains.
void launch_hsppeel_chain_key_major(const HspPeelArgs& a, const uint32_t* idx, hipStream_t s);
// keep[c] for chain position c, keep[n] = 0; tot[2] = the number of heads.
void launch_hsppeel_keep(const HspPeelArgs& a, hipStream_t s);
// cpos[corder[c]] = c, khead[kidx[c]] = corder[c] for a kept chain.
void launch_hsppeel_assign(const HspPeelArgs& a, hipStream_t s);
// key_a[r] = the kept chain of node r (NONE for a dropped chain's node), idx_a[r] = r, chain_of[order[r]] likewise.
void launch_hsppeel_node_key(const HspPeelArgs& a, hipStream_t s);
// From the nodes sorted by chain (key, idx): the member records and first[].
void launch_hsppeel_members(const HspPeelArgs& a, const uint64_t* key, const uint32_t* idx, hipStream_t s);
// The chain records of the kept chains, and tot[0], tot[1].
void launch_hsppeel_records(const HspPeelArgs& a, hipStream_t s);

}  // namespace sa
