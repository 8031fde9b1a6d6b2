// pmx_align_chain_probe (include/panmap_amd.h) and hs_chain_probe (tests/hostsim): the parts the device kernels and the CPU
// unit-test build share -- the parameter block with its defaults, and the dispatcher that runs one operation of the sort /
// chaining code on a bound Work exactly as map_frag (aln_map.hpp) calls it.  TEST ACCESSOR: nothing on the product path
// includes this file.
#pragma once
#include "aln_rmq.hpp"

namespace pmx {
namespace aln {

enum { PMX_CP_SORT128 = 0, PMX_CP_SORT64 = 1, PMX_CP_CHAIN_DP = 2, PMX_CP_CHAIN_RMQ = 3 };
#define PMX_CP_DEFAULT INT32_MIN   // an integer parameter left to the preset (a float: NaN)

// == pmx_chain_probe_params
struct ChainProbeParams {
    int32_t bw, bw_long, max_gap, max_chain_skip, max_chain_iter, min_cnt, min_chain_score;
    float chn_pen_gap, chn_pen_skip;
    int32_t rmq_inner_dist, rmq_size_cap, max_dist_x, max_dist_y, n_seg;
};

// the preset's value wherever the caller left the default, written back to `p`; the overrides into a copy of the options
inline Opt chain_probe_resolve(ChainProbeParams& p, const Opt& preset) {
    Opt o = preset;
    auto pick = [](int32_t& v, int& field) { if (v == PMX_CP_DEFAULT) v = field; else field = v; };
    pick(p.bw, o.bw); pick(p.bw_long, o.bw_long); pick(p.max_gap, o.max_gap); pick(p.max_chain_skip, o.max_chain_skip);
    pick(p.max_chain_iter, o.max_chain_iter); pick(p.min_cnt, o.min_cnt); pick(p.min_chain_score, o.min_chain_score);
    pick(p.rmq_inner_dist, o.rmq_inner_dist); pick(p.rmq_size_cap, o.rmq_size_cap);
    if (p.chn_pen_gap != p.chn_pen_gap) p.chn_pen_gap = o.chn_pen_gap; else o.chn_pen_gap = p.chn_pen_gap;
    if (p.chn_pen_skip != p.chn_pen_skip) p.chn_pen_skip = o.chn_pen_skip; else o.chn_pen_skip = p.chn_pen_skip;
    // map_frag's max_chain_gap_ref / max_chain_gap_qry of a read without a fragment-length limit
    if (p.max_dist_x == PMX_CP_DEFAULT) p.max_dist_x = o.max_gap;
    if (p.max_dist_y == PMX_CP_DEFAULT) p.max_dist_y = o.max_gap;
    if (p.n_seg == PMX_CP_DEFAULT) p.n_seg = 1;
    return o;
}

// W.a[0 .. W.n_a) holds the list (SORT64: W.a viewed as 64-bit words holds W.n_a values), W.n_segs / W.qlen[] are set
PMX_HD void chain_probe_run(Work& W, const Opt& o, int op, int max_dist_x, int max_dist_y, int n_seg) {
    W.n_u = 0;
    if (op == PMX_CP_SORT128) {
        Ptr<A128> a = W.a;
        radix_sort_128x(a, a + W.n_a, &W.status);
    } else if (op == PMX_CP_SORT64) {
        Ptr<uint64_t> v = ptr_cast<uint64_t>(W.a);
        radix_sort_64(v, v + W.n_a, &W.status);
    } else if (op == PMX_CP_CHAIN_DP) {
        chain_dp(W, o, max_dist_x, max_dist_y, n_seg);
    } else {
        chain_rmq(W, o.max_gap, o.rmq_inner_dist, o.bw_long, o.max_chain_skip, o.rmq_size_cap, o.min_cnt, o.min_chain_score, o.chn_pen_gap, o.chn_pen_skip);
    }
}

// per list (== pmx_chain_probe_result)
struct ChainProbeOut {
    int32_t served;
    uint32_t status;
    int64_t n_a;
    int32_t n_u, pad;
};

}  // namespace aln
}  // namespace pmx
