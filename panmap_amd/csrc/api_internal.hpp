// Shared internals of the C ABI translation units.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/panmap_amd.h"

namespace pmx {
void set_error(const std::string& s);
struct LiteIndex;
}  // namespace pmx

// host-side accessors used by the device TU
const pmx::LiteIndex* pmx_index_internal(const pmx_index* idx);

// the multi-GPU transport for the --meta unit (api_dist.hip; not part of the C ABI).  Both are collective and throw on failure.
namespace pmx {
pmx_ctx* dist_ctx(const pmx_dist* d);
// every rank's `bytes` bytes of device memory at d_mine, rank-major, into d_all (world * bytes); stream-ordered on the context's stream
void dist_all_gather(pmx_dist* d, const void* d_mine, size_t bytes, void* d_all);
// rank r's sizes[r] bytes of device memory at d_mine to offset offs[r] of d_all on `root` (the root's own part included); every rank calls it
void dist_gather_v(pmx_dist* d, const void* d_mine, const std::vector<size_t>& sizes, const std::vector<size_t>& offs, void* d_all, int root);
// every rank's k int64 values -> host, rank-major
std::vector<int64_t> dist_exchange_counts(pmx_dist* d, const int64_t* mine, int k);
}  // namespace pmx
