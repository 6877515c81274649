// The layout stage (b4): the flat witness streams into the columns of the circuit.  The break points of the advice stream from its
// gate-start bits, the advice and lookup columns (materialised, or as column sources the NTT and the MSM read through), the column
// images of the constant-cell flags and of the gate selectors, and the split of a column's scalars by that mask.  The streams are read
// once here; nothing in this file knows a gadget, a table or a witness call's context.
#include <vector>

#include "hostglue.hpp"

namespace vdb {

// ------------------------------------------------------------------ kernels (halo2-base assign_threads_in)
// break points from the gate-start bits: the row walk of GateThreadBuilder::assign_all.  A column that
// starts at stream cell S breaks at the first row r in {M-3, M-2 (if that cell starts a gate), M-1}.
__global__ void k_layout_plan(const uint8_t* __restrict__ sel, uint64_t n_cells, uint64_t max_rows, uint64_t* __restrict__ bp, uint64_t cap,
                              uint64_t* __restrict__ n_bp) {
  if (blockIdx.x || threadIdx.x) return;
  uint64_t S = 0, cnt = 0;
  const uint64_t M = max_rows;
  for (;;) {
    uint64_t r;
    if (M >= 3 && S + M - 3 < n_cells && (sel[S + M - 3] & 1)) r = M - 3;
    else if (M >= 2 && S + M - 2 < n_cells && (sel[S + M - 2] & 1)) r = M - 2;
    else r = M - 1;
    if (S + r >= n_cells) break;
    if (cnt < cap) bp[cnt] = r;
    cnt++;
    S += r;
  }
  *n_bp = cnt;
}
__global__ __launch_bounds__(256) void k_layout_columns(const u256* __restrict__ stream, uint64_t n_cells, const uint64_t* __restrict__ starts,
                                                        const uint64_t* __restrict__ bp, uint64_t n_bp, uint32_t k, u256* __restrict__ cols,
                                                        const u256* __restrict__ blind, uint32_t n_blind, uint64_t col_lo, uint64_t col_hi) {
  const uint64_t rows = 1ull << k;
  uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t total = (col_hi - col_lo) * rows;
  if (idx >= total) return;
  uint64_t col = col_lo + (idx >> k), row = idx & (rows - 1);
  uint64_t start = starts[col];
  uint64_t len = col < n_bp ? bp[col] + 1 : n_cells - start;  // cells held by this column
  u256 v = u256_zero();
  if (row < len) v = ld256(stream + start + row);
  else if (blind && row >= rows - n_blind) v = ld256(blind + col * n_blind + (row - (rows - n_blind)));
  st256(cols + idx, v);
}
__global__ __launch_bounds__(256) void k_layout_lookup(const u256* __restrict__ lk, uint64_t n_cells, uint64_t max_rows, uint32_t k, uint64_t n_cols,
                                                       u256* __restrict__ cols, const u256* __restrict__ blind, uint32_t n_blind, uint64_t col_lo) {
  const uint64_t rows = 1ull << k;
  uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_cols * rows) return;
  uint64_t col = col_lo + (idx >> k), row = idx & (rows - 1);
  uint64_t src = col * max_rows + row;
  u256 v = u256_zero();
  if (row < max_rows && src < n_cells) v = ld256(lk + src);
  else if (blind && row >= rows - n_blind) v = ld256(blind + col * n_blind + (row - (rows - n_blind)));
  st256(cols + idx, v);
}

// column-layout image of the constant-cell flags (bit 1 of the keygen flag byte): mask[col][row] = 1 when the cell
// laid out there is a data-independent constant
__global__ __launch_bounds__(256) void k_layout_const_mask(const uint8_t* __restrict__ flags, uint64_t n_cells, const uint64_t* __restrict__ starts,
                                                           const uint64_t* __restrict__ bp, uint64_t n_bp, uint32_t k, uint8_t* __restrict__ mask) {
  const uint64_t rows = 1ull << k;
  uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (n_bp + 1) * rows) return;
  uint64_t col = idx >> k, row = idx & (rows - 1);
  uint64_t start = starts[col];
  uint64_t len = col < n_bp ? bp[col] + 1 : n_cells - start;
  mask[idx] = row < len ? (flags[start + row] >> 1) & 1 : 0;
}
// column-layout image of the gate selectors as field elements: q[col][row] = 1 where a gate starts (bit 0 of the flag byte)
__global__ __launch_bounds__(256) void k_layout_selectors(const uint8_t* __restrict__ flags, uint64_t n_cells, const uint64_t* __restrict__ starts,
                                                          const uint64_t* __restrict__ bp, uint64_t n_bp, uint32_t k, u256* __restrict__ q) {
  const uint64_t rows = 1ull << k;
  uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (n_bp + 1) * rows) return;
  uint64_t col = idx >> k, row = idx & (rows - 1);
  uint64_t start = starts[col];
  uint64_t len = col < n_bp ? bp[col] + 1 : n_cells - start;
  // the last cell of a column that is not the last one is the cell the next column starts with again (break points sit on
  // gate boundaries: it closes a gate here and opens one there), so its selector is enabled in the next column only
  const uint64_t sel_len = col < n_bp ? len - 1 : len;
  st256(q + idx, (row < sel_len && (flags[start + row] & 1)) ? mont_one<Fr>() : u256_zero());
}
// scalars' = mask ? v : 0 (constant part) or mask ? 0 : v (variable part)
__global__ __launch_bounds__(256) void k_mask_select(const u256* __restrict__ in, const uint8_t* __restrict__ mask, uint64_t n, int keep_const,
                                                     u256* __restrict__ out) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool m = mask[i] != 0;
  st256(out + i, (m == (keep_const != 0)) ? ld256(in + i) : u256_zero());
}

}  // namespace vdb

using namespace vdb;

// break points and their prefix sums (column c starts at stream cell starts[c]) -> device scratch slot 1
static int upload_break_points(const uint64_t* break_points, uint64_t n_bp, uint64_t** dbp, uint64_t** dstarts) {
  static thread_local std::vector<uint64_t> h;  // pageable source: hipMemcpyAsync stages it before returning
  h.resize(2 * n_bp + 2);
  uint64_t acc = 0;
  h[n_bp] = 0;
  for (uint64_t i = 0; i < n_bp; i++) {
    h[i] = break_points[i];
    acc += break_points[i];
    h[n_bp + 1 + i] = acc;
  }
  uint64_t* d = (uint64_t*)scratch_get(1, (2 * n_bp + 2) * sizeof(uint64_t));
  if (!d) return VDB_ERR_OOM;
  VDB_HIP(hipMemcpyAsync(d, h.data(), (2 * n_bp + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx().stream));
  *dbp = d;
  *dstarts = d + n_bp;
  return VDB_OK;
}

extern "C" {

int vdb_layout_plan_dev(const uint8_t* selector_dev, uint64_t n_cells, uint32_t k, uint32_t minimum_rows, uint64_t* break_points_out, uint64_t cap,
                        uint64_t* n_break_points) {
  VDB_REQUIRE_INIT();
  VDB_ARG(selector_dev && n_break_points && k >= 3 && k <= 28 && ((uint64_t)1 << k) > minimum_rows + 4, "bad argument");
  uint64_t max_rows = ((uint64_t)1 << k) - minimum_rows;
  uint64_t est = n_cells / (max_rows - 3) + 2;
  uint64_t* d = (uint64_t*)scratch_get(1, (est + 1) * sizeof(uint64_t));
  if (!d) return VDB_ERR_OOM;
  VDB_LAUNCH(k_layout_plan, dim3(1), dim3(1), selector_dev, n_cells, max_rows, d + 1, est, d);
  uint64_t nbp = 0;
  VDB_HIP(hipMemcpyAsync(&nbp, d, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx().stream));
  VDB_HIP(hipStreamSynchronize(ctx().stream));
  *n_break_points = nbp;
  if (break_points_out) {
    VDB_ARG(cap >= nbp, "break point buffer too small");
    VDB_HIP(hipMemcpy(break_points_out, d + 1, nbp * sizeof(uint64_t), hipMemcpyDeviceToHost));
  }
  return VDB_OK;
}
int vdb_layout_plan(const uint8_t* selector, uint64_t n_cells, uint32_t k, uint32_t minimum_rows, uint64_t* break_points_out, uint64_t cap,
                    uint64_t* n_break_points) {
  VDB_REQUIRE_INIT();
  VDB_ARG(selector, "null pointer");
  DevBuf ds;
  TRY(upload(ds, selector, n_cells));
  return vdb_layout_plan_dev(ds.as<uint8_t>(), n_cells, k, minimum_rows, break_points_out, cap, n_break_points);
}
int vdb_layout_columns_dev(const vdb_fr* stream_dev, uint64_t n_cells, const uint64_t* break_points, uint64_t n_bp, uint32_t k, vdb_fr* cols_dev,
                           const vdb_fr* blind_dev, uint32_t n_blind) {
  return vdb_layout_columns_range_dev(stream_dev, n_cells, break_points, n_bp, k, 0, n_bp + 1, cols_dev, blind_dev, n_blind);
}
int vdb_layout_columns_range_dev(const vdb_fr* stream_dev, uint64_t n_cells, const uint64_t* break_points, uint64_t n_bp, uint32_t k, uint64_t col_lo,
                                 uint64_t col_hi, vdb_fr* cols_dev, const vdb_fr* blind_dev, uint32_t n_blind) {
  VDB_REQUIRE_INIT();
  VDB_ARG(stream_dev && cols_dev && (break_points || n_bp == 0) && k <= 28 && col_lo <= col_hi && col_hi <= n_bp + 1, "bad argument");
  if (col_lo == col_hi) return VDB_OK;
  const uint64_t rows = 1ull << k;
  uint64_t sum = 0;
  for (uint64_t i = 0; i < n_bp; i++) {
    VDB_ARG(break_points[i] < rows, "break point beyond the column height");
    sum += break_points[i];
  }
  VDB_ARG(sum <= n_cells && n_cells - sum <= rows, "break points do not match the stream length");
  uint64_t *dbp, *dst;
  TRY(upload_break_points(break_points, n_bp, &dbp, &dst));
  uint64_t total = (col_hi - col_lo) * rows;
  VDB_LAUNCH(k_layout_columns, dim3((unsigned)((total + 255) / 256)), dim3(256), as_u256(stream_dev), n_cells, dst, dbp, n_bp, k, as_u256(cols_dev),
             blind_dev ? as_u256(blind_dev) : nullptr, n_blind, col_lo, col_hi);
  VDB_HIP(hipStreamSynchronize(ctx().stream));  // break_points is a host buffer the caller may free
  return VDB_OK;
}
int vdb_colsrc_build_dev(const vdb_fr* stream_dev, uint64_t n_cells, const uint64_t* break_points, uint64_t n_bp, uint32_t k, uint64_t col_lo,
                         uint64_t col_hi, const vdb_fr* blind_dev, uint32_t n_blind, vdb_colsrc* out_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(stream_dev && out_dev && (break_points || n_bp == 0) && k <= 28 && col_lo <= col_hi && col_hi <= n_bp + 1, "bad argument");
  const uint64_t rows = 1ull << k;
  std::vector<vdb_colsrc> h(col_hi - col_lo);
  uint64_t start = 0;
  for (uint64_t c = 0; c < col_hi; c++) {
    if (c < n_bp) VDB_ARG(break_points[c] < rows, "break point beyond the column height");
    const uint64_t len = c < n_bp ? break_points[c] + 1 : n_cells - start;
    VDB_ARG(start <= n_cells && len <= rows && start + len <= n_cells, "break points do not match the stream length");
    if (c >= col_lo) {
      // colsrc_fetch (and k_layout_columns) read a row below len from the stream before they look at the blinding rows
      VDB_ARG(!blind_dev || len + n_blind <= rows, "a column's cells reach into its blinding rows");
      h[c - col_lo].src = stream_dev + start;
      h[c - col_lo].len = len;
      h[c - col_lo].blind = blind_dev ? blind_dev + c * n_blind : nullptr;
    }
    if (c < n_bp) start += break_points[c];
  }
  if (!h.empty()) VDB_HIP(hipMemcpyAsync(out_dev, h.data(), h.size() * sizeof(vdb_colsrc), hipMemcpyHostToDevice, ctx().stream));
  VDB_HIP(hipStreamSynchronize(ctx().stream));
  return VDB_OK;
}
int vdb_colsrc_build_lookup_dev(const vdb_fr* lookup_dev, uint64_t n_cells, uint32_t k, uint32_t minimum_rows, uint64_t col_lo, uint64_t col_hi,
                                const vdb_fr* blind_dev, uint32_t n_blind, vdb_colsrc* out_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(out_dev && (lookup_dev || n_cells == 0) && k <= 28 && col_lo <= col_hi && minimum_rows < (1u << k), "bad argument");
  const uint64_t max_rows = (1ull << k) - minimum_rows;
  std::vector<vdb_colsrc> h(col_hi - col_lo);
  for (uint64_t c = col_lo; c < col_hi; c++) {
    const uint64_t start = c * max_rows;
    h[c - col_lo].src = lookup_dev + (start < n_cells ? start : 0);
    h[c - col_lo].len = start < n_cells ? (n_cells - start < max_rows ? n_cells - start : max_rows) : 0;
    VDB_ARG(!blind_dev || h[c - col_lo].len + n_blind <= (1ull << k), "a column's cells reach into its blinding rows");
    h[c - col_lo].blind = blind_dev ? blind_dev + c * n_blind : nullptr;
  }
  if (!h.empty()) VDB_HIP(hipMemcpyAsync(out_dev, h.data(), h.size() * sizeof(vdb_colsrc), hipMemcpyHostToDevice, ctx().stream));
  VDB_HIP(hipStreamSynchronize(ctx().stream));
  return VDB_OK;
}
int vdb_layout_lookup_dev(const vdb_fr* lookup_dev, uint64_t n_cells, uint32_t k, uint32_t minimum_rows, vdb_fr* cols_dev, uint64_t n_cols,
                          const vdb_fr* blind_dev, uint32_t n_blind) {
  VDB_ARG(n_cols * ((((uint64_t)1 << k)) - minimum_rows) >= n_cells, "not enough lookup columns");
  return vdb_layout_lookup_range_dev(lookup_dev, n_cells, k, minimum_rows, 0, n_cols, cols_dev, blind_dev, n_blind);
}
int vdb_layout_lookup_range_dev(const vdb_fr* lookup_dev, uint64_t n_cells, uint32_t k, uint32_t minimum_rows, uint64_t col_lo, uint64_t col_hi,
                                vdb_fr* cols_dev, const vdb_fr* blind_dev, uint32_t n_blind) {
  VDB_REQUIRE_INIT();
  VDB_ARG(cols_dev && (lookup_dev || n_cells == 0) && k <= 28 && col_lo <= col_hi, "bad argument");
  uint64_t max_rows = ((uint64_t)1 << k) - minimum_rows;
  const uint64_t n_cols = col_hi - col_lo;
  if (n_cols == 0) return VDB_OK;
  uint64_t total = n_cols << k;
  VDB_LAUNCH(k_layout_lookup, dim3((unsigned)((total + 255) / 256)), dim3(256), as_u256(lookup_dev), n_cells, max_rows, k, n_cols, as_u256(cols_dev),
             blind_dev ? as_u256(blind_dev) : nullptr, n_blind, col_lo);
  return VDB_OK;
}
int vdb_layout_const_mask_dev(const uint8_t* flags_dev, uint64_t n_cells, const uint64_t* break_points, uint64_t n_bp, uint32_t k, uint8_t* mask_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(flags_dev && mask_dev && (break_points || n_bp == 0) && k <= 28, "bad argument");
  const uint64_t rows = 1ull << k;
  uint64_t *dbp, *dst;
  TRY(upload_break_points(break_points, n_bp, &dbp, &dst));
  uint64_t total = (n_bp + 1) * rows;
  VDB_LAUNCH(k_layout_const_mask, dim3((unsigned)((total + 255) / 256)), dim3(256), flags_dev, n_cells, dst, dbp, n_bp, k, mask_dev);
  VDB_HIP(hipStreamSynchronize(ctx().stream));
  return VDB_OK;
}
int vdb_layout_selectors_dev(const uint8_t* flags_dev, uint64_t n_cells, const uint64_t* break_points, uint64_t n_bp, uint32_t k, vdb_fr* q_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(flags_dev && q_dev && (break_points || n_bp == 0) && k <= 28, "bad argument");
  const uint64_t rows = 1ull << k;
  uint64_t *dbp, *dst;
  TRY(upload_break_points(break_points, n_bp, &dbp, &dst));
  uint64_t total = (n_bp + 1) * rows;
  VDB_LAUNCH(k_layout_selectors, dim3((unsigned)((total + 255) / 256)), dim3(256), flags_dev, n_cells, dst, dbp, n_bp, k, as_u256(q_dev));
  VDB_HIP(hipStreamSynchronize(ctx().stream));
  return VDB_OK;
}
int vdb_mask_select_dev(const vdb_fr* in_dev, const uint8_t* mask_dev, uint64_t n, int keep_const, vdb_fr* out_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(in_dev && mask_dev && out_dev, "null pointer");
  if (n == 0) return VDB_OK;
  VDB_LAUNCH(k_mask_select, dim3((unsigned)((n + 255) / 256)), dim3(256), as_u256(in_dev), mask_dev, n, keep_const, as_u256(out_dev));
  return VDB_OK;
}
int vdb_layout_columns(const vdb_fr* stream, uint64_t n_cells, const uint64_t* break_points, uint64_t n_bp, const vdb_fr* lookup, uint64_t n_lookup,
                       uint32_t k, uint32_t minimum_rows, vdb_fr* advice_cols_out, vdb_fr* lookup_cols_out, uint64_t n_lookup_cols) {
  VDB_REQUIRE_INIT();
  VDB_ARG(stream && advice_cols_out, "null pointer");
  const uint64_t rows = 1ull << k;
  DevBuf ds, dc, dl, dlc;
  TRY(upload(ds, stream, n_cells * sizeof(u256)));
  TRY(dc.alloc((n_bp + 1) * rows * sizeof(u256)));
  TRY(vdb_layout_columns_dev(ds.as<vdb_fr>(), n_cells, break_points, n_bp, k, dc.as<vdb_fr>(), nullptr, 0));
  TRY(download(advice_cols_out, dc.p, (n_bp + 1) * rows * sizeof(u256)));
  if (lookup_cols_out && n_lookup_cols) {
    TRY(upload(dl, lookup, n_lookup * sizeof(u256)));
    TRY(dlc.alloc(n_lookup_cols * rows * sizeof(u256)));
    TRY(vdb_layout_lookup_dev(dl.as<vdb_fr>(), n_lookup, k, minimum_rows, dlc.as<vdb_fr>(), n_lookup_cols, nullptr, 0));
    TRY(download(lookup_cols_out, dlc.p, n_lookup_cols * rows * sizeof(u256)));
  }
  VDB_HIP(hipStreamSynchronize(ctx().stream));
  return VDB_OK;
}

}  // extern "C"
