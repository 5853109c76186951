// The host side that ksh_kss_pair_counts, ksh_kss_select_* and ksh_kss_color_classes share (ksh_rowtile.h): the
// column list of a call, the projection of the ancestor rows onto it, the prologue and the launch of a walk.
#include "ksh_rowtile.h"

#include <algorithm>

using namespace ksh::pc;

namespace ksh {

int check_col_count(const int32_t* cols, int32_t n_cols, const char* name) {
  if (cols && (n_cols < 1 || n_cols > kMaxCols))
    return fail(KSH_INVALID_ARGUMENT, "n_cols = %d (the length of %s) is outside [1, %d]", n_cols, name, kMaxCols);
  return KSH_OK;
}

int resolve_cols(const int32_t* cols, int32_t n_cols, const IndexShape& x, const char* name, ColList* list,
                 int* n_out, std::vector<int>* col_of) {
  std::vector<int> mine, &at = col_of ? *col_of : mine;
  at.assign(size_t(x.n_nodes), -1);
  if (!cols) {
    if (x.n_nodes > kMaxCols)
      return fail(KSH_INVALID_ARGUMENT, "%s is NULL (all nodes) but the index has %d nodes, more than %d columns: "
                                        "name the columns of each call", name, x.n_nodes, kMaxCols);
    n_cols = x.n_nodes;
    for (int32_t c = 0; c < n_cols; c++) list->id[c] = at[size_t(c)] = c;
  } else {
    for (int32_t c = 0; c < n_cols; c++) {
      const int32_t id = cols[c];
      if (id < 0 || id >= x.n_nodes)
        return fail(KSH_INVALID_ARGUMENT, "%s[%d] = %d is outside [0, %d)", name, c, id, x.n_nodes);
      if (at[size_t(id)] >= 0) return fail(KSH_INVALID_ARGUMENT, "%s[%d] = %d is repeated", name, c, id);
      at[size_t(id)] = c;
      list->id[c] = id;
    }
  }
  *n_out = n_cols;
  return KSH_OK;
}

__global__ __launch_bounds__(256) void k_pair_project(const uint64_t* __restrict__ anc, int wt, int n_nodes,
                                                      ColList cols, int n_cols, uint64_t* __restrict__ proj) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_nodes) return;
  uint64_t w[2] = {0, 0};
  for (int c = 0; c < n_cols; c++) {
    const int id = cols.id[c];
    w[c >> 6] |= ((anc[size_t(j) * wt + (id >> 6)] >> (id & 63)) & 1) << (c & 63);
  }
  proj[2 * j] = w[0];
  proj[2 * j + 1] = w[1];
}

static int pair_project(ksh_ctx* ctx, const IndexShape& x, const ColList& cols, int n_cols, uint64_t* proj) {
  hipLaunchKernelGGL(k_pair_project, dim3(unsigned((x.n_nodes + 255) / 256)), dim3(256), 0, ctx->stream, x.d_anc,
                     x.wt, x.n_nodes, cols, n_cols, proj);
  KSH_HIP(hipGetLastError());
  return KSH_OK;
}

int walk_prologue(ksh_kss_index* idx, const IndexShape& x, const ColList& cols, int n_cols, PoolBuf* proj) {
  KSH_HIP(hipSetDevice(x.ctx->device));
  KSH_TRY(pool_alloc(x.ctx, size_t(std::max(x.n_nodes, 1)) * 16, &proj->p));
  index_set_routes(idx, 0);
  KSH_HIP(hipMemsetAsync(x.d_flags, 0, 16, x.ctx->stream));
  return pair_project(x.ctx, x, cols, n_cols, static_cast<uint64_t*>(proj->p));
}

int walk_grid(ksh_ctx* ctx, const IndexShape& x, const void* kernel, size_t lds, size_t lds_max, uint32_t opt_in,
              unsigned* grid) {
  if (lds_max > (64u << 10) && !(ctx->lds_opt_in & opt_in)) {  // (more than the 64 KB a kernel gets without asking)
    KSH_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_max)));
    ctx->lds_opt_in |= opt_in;
  }
  int n_cu = 0;
  KSH_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device));
  const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(2, int64_t(160 << 10) / int64_t(lds)));
  const int64_t want = (x.total_keys + kRowsPerGroup - 1) / kRowsPerGroup;
  *grid = unsigned(std::max<int64_t>(1, std::min({want, int64_t(n_buckets(&x.g)), per_cu * n_cu})));
  return KSH_OK;
}

}  // namespace ksh
