// Presort of a boosting stage's variables on gfx950 (section 6 of the C ABI): everything that makes the sorted tables of the
// split search (cc_split.hip) or accounts for their memory. cc_eval_presort keeps every variable's table resident for the
// stage; cc_eval_presort_split keeps a head of them and leaves the rest to the streamed tail of the search, which fills one
// chunk table at a time through the same pass (fill_sorted_table).
//
// Data layout in HBM: variables in groups of 64; per group the sorted values (f32) and sample indices (u16 when
// n_samples <= 65 536, else i32) are interleaved [group][rank][64 lanes] (SortedTable), so that lane = variable reads of one rank
// are one coalesced 256-B / 128-B segment. LBP: category codes u8 [variable][sample] and the table of k_split_cat_sorted.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>

#include "cc_eval_internal.h"

namespace ccamd {

// ------------------------------------------------------------------------------------------------
// [rows][n] row-major (one sorted variable per row) -> [group][rank][64]
// ------------------------------------------------------------------------------------------------
template <class TI>
__global__ __launch_bounds__(256) void k_interleave(const float* __restrict__ vals, const int* __restrict__ idx, int rows, int n,
                                                    float* __restrict__ out_val, TI* __restrict__ out_idx, size_t group0) {
  __shared__ float tv[64][65];
  __shared__ int ti[64][65];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.x * 64, g = blockIdx.y;
  for (int j = wave; j < 64; j += 4) {
    const int row = g * 64 + j;
    float v = 0.f;
    int s = 0;
    if (row < rows && r0 + lane < n) {
      v = vals[(size_t)row * n + r0 + lane];
      s = idx[(size_t)row * n + r0 + lane];
    }
    tv[j][lane] = v;
    ti[j][lane] = s;
  }
  __syncthreads();
  for (int rr = wave; rr < 64; rr += 4) {
    if (r0 + rr >= n) break;
    const size_t o = ((group0 + g) * (size_t)n + r0 + rr) * 64 + lane;
    out_val[o] = tv[lane][rr];
    out_idx[o] = (TI)ti[lane][rr];
  }
}

// ------------------------------------------------------------------------------------------------
// Stable sort of every row of [rows][n] (one variable per row) with the sample position as the value: one block of 1024
// threads per row, the whole row in registers + LDS (hipcub::BlockRadixSort: LSD radix, stable -- equal values keep
// increasing sample order, what std::stable_sort over (value, index) gives the reference,
// o_cvcascadeboosttraindata.cpp:582-596). A row of a boosting stage (<= 24 576 samples) fits a CU's LDS, so it is read
// once and written once: 8 B + 8 B per element instead of the ~70 B of a device-wide segmented radix sort's four passes.
// ------------------------------------------------------------------------------------------------
constexpr int SORT_THREADS = 1024;
template <int ITEMS>
struct RowSort {
  using Sort = hipcub::BlockRadixSort<float, SORT_THREADS, ITEMS, unsigned short>;
  static constexpr size_t lds_bytes = sizeof(typename Sort::TempStorage);
};
template <int ITEMS>
__global__ __launch_bounds__(SORT_THREADS) void k_sort_rows_block(const float* __restrict__ vals, int rows, int n, float* __restrict__ keys_out,
                                                                  int* __restrict__ idx_out) {
  extern __shared__ __attribute__((aligned(16))) char sort_lds[];
  using Sort = typename RowSort<ITEMS>::Sort;
  typename Sort::TempStorage& temp = *reinterpret_cast<typename Sort::TempStorage*>(sort_lds);
  const int row = blockIdx.x;
  if (row >= rows) return;
  const float* src = vals + (size_t)row * n;
  float key[ITEMS];
  unsigned short val[ITEMS];
#pragma unroll
  for (int i = 0; i < ITEMS; i++) {  // blocked arrangement: thread t owns positions t * ITEMS ..
    const int pos = (int)threadIdx.x * ITEMS + i;
    // padding = +inf: sorts behind every finite value. Precondition: no NaN among the values (a NaN's radix key sorts behind
    // +inf and would push padding into the first n ranks). The evaluators cannot produce one: Haar values are finite sums
    // divided by a positive norm factor or 0 when it is 0 (haarfeatures.h:108-112), LBP codes are 0..255.
    key[i] = pos < n ? src[pos] : __int_as_float(0x7f800000);
    val[i] = (unsigned short)pos;
  }
  Sort(temp).SortBlockedToStriped(key, val);
#pragma unroll
  for (int i = 0; i < ITEMS; i++) {  // striped: rank = i * 1024 + t, consecutive lanes write consecutive ranks
    const int rank = i * SORT_THREADS + (int)threadIdx.x;
    if (rank < n) {
      keys_out[(size_t)row * n + rank] = key[i];
      idx_out[(size_t)row * n + rank] = (int)val[i];
    }
  }
}
template <int ITEMS>
static hipError_t launch_sort_rows_block(const float* vals, int rows, int n, float* keys_out, int* idx_out, hipStream_t st) {
  constexpr size_t lds = RowSort<ITEMS>::lds_bytes;
  if (lds > 64 * 1024) {
    // The opt-in is per device and cheap: set it on every launch (a process-wide "done" flag, as round 3 kept, leaves the
    // second device of a process without it, and is not thread-safe).
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sort_rows_block<ITEMS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((k_sort_rows_block<ITEMS>), dim3((unsigned)rows), dim3(SORT_THREADS), lds, st, vals, rows, n, keys_out, idx_out);
  return hipGetLastError();
}

int sort_rows_block_limit() { return SORT_THREADS * 24; }
hipError_t sort_rows_block(const float* vals, int rows, int n, float* keys_out, int* idx_out, hipStream_t st) {
  if (n <= SORT_THREADS * 4) return launch_sort_rows_block<4>(vals, rows, n, keys_out, idx_out, st);
  if (n <= SORT_THREADS * 8) return launch_sort_rows_block<8>(vals, rows, n, keys_out, idx_out, st);
  if (n <= SORT_THREADS * 12) return launch_sort_rows_block<12>(vals, rows, n, keys_out, idx_out, st);
  if (n <= SORT_THREADS * 16) return launch_sort_rows_block<16>(vals, rows, n, keys_out, idx_out, st);
  if (n <= SORT_THREADS * 20) return launch_sort_rows_block<20>(vals, rows, n, keys_out, idx_out, st);
  return launch_sort_rows_block<24>(vals, rows, n, keys_out, idx_out, st);
}

__global__ void k_codes_u8(const float* __restrict__ in, uint8_t* __restrict__ out, size_t total) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) out[i] = (uint8_t)(int)in[i];
}

__global__ void k_iota_rows2(int* __restrict__ v, size_t total, int n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) v[i] = (int)(i % (size_t)n);
}

// [rows][n] sorted codes (as floats) and sample positions -> (sample << 8 | code) as [group][rank / 4][64][4]
__global__ __launch_bounds__(256) void k_interleave_cat(const float* __restrict__ vals, const int* __restrict__ idx, int rows, int n,
                                                        uint32_t* __restrict__ out, size_t group0) {
  __shared__ uint32_t tv[64][65];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.x * 64, g = blockIdx.y;
  for (int j = wave; j < 64; j += 4) {
    const int row = g * 64 + j;
    uint32_t v = 0;
    if (row < rows && r0 + lane < n) v = ((uint32_t)idx[(size_t)row * n + r0 + lane] << 8) | ((uint32_t)(int)vals[(size_t)row * n + r0 + lane] & 255u);
    tv[j][lane] = v;
  }
  __syncthreads();
  const size_t n4 = ((size_t)n + 3) >> 2;
  for (int rr = wave; rr < 64; rr += 4) {  // [group][rank / 4][lane][rank % 4]; r0 is a multiple of 64
    if (r0 + rr >= n) break;
    out[(((group0 + g) * n4 + ((r0 + rr) >> 2)) * 64 + lane) * 4 + (rr & 3)] = tv[lane][rr];
  }
}

}  // namespace ccamd

using namespace ccamd;

// RowSorter (cc_eval_internal.h): the scratch of one pass and its two sorts.
cc_status RowSorter::init() {
  CC_HIP(e->d_out.ensure((size_t)FB * N));
  CC_HIP(keys_out.ensure((size_t)FB * N));
  CC_HIP(sorted.ensure((size_t)FB * N));
  return CC_OK;
}
cc_status RowSorter::prepare_segmented() {
  if (segmented_ready) return CC_OK;
  const size_t cap = (size_t)FB * N;
  CC_HIP(iota.ensure(cap));
  CC_HIP(offsets.ensure((size_t)FB + 1));
  std::vector<int> off((size_t)FB + 1);
  for (int i = 0; i <= FB; i++) off[(size_t)i] = (int)((size_t)i * N);
  CC_HIP(hipMemcpyAsync(offsets.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, e->stream.s));
  CC_HIP(hipStreamSynchronize(e->stream.s));  // `off` is pageable and about to go out of scope
  hipLaunchKernelGGL(k_iota_rows2, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, e->stream.s, iota.p, cap, N);
  segmented_ready = true;
  return CC_OK;
}
cc_status RowSorter::sort(int nf) {
  if (N <= sort_rows_block_limit()) {  // a row fits one block: sorted in LDS, read once and written once
    // a part that refuses the ~100 KB LDS request (or the launch) takes the device-wide sort below instead of failing
    if (sort_rows_block(e->d_out.p, nf, N, keys_out.p, sorted.p, e->stream.s) == hipSuccess) return CC_OK;
    (void)hipGetLastError();
  }
  if (cc_status st = prepare_segmented(); st != CC_OK) return st;
  const size_t total = (size_t)nf * N;
  size_t temp_bytes = 0;
  CC_HIP(hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, temp_bytes, e->d_out.p, keys_out.p, iota.p, sorted.p, (int)total, nf, offsets.p,
                                                     offsets.p + 1, 0, 32, e->stream.s));
  CC_HIP(temp.ensure(std::max<size_t>(temp_bytes, 1)));
  // stable: equal values keep increasing sample order
  CC_HIP(hipcub::DeviceSegmentedRadixSort::SortPairs(temp.p, temp_bytes, e->d_out.p, keys_out.p, iota.p, sorted.p, (int)total, nf, offsets.p,
                                                     offsets.p + 1, 0, 32, e->stream.s));
  return CC_OK;
}

cc_status SortedTable::alloc(size_t entries, bool wide_, hipStream_t st) {
  wide = wide_;
  CC_HIP(val.ensure(entries + PAD));
  CC_HIP(wide ? idx32.ensure(entries + PAD) : idx16.ensure(entries + PAD));
  return zero_padding(entries, st);
}
cc_status SortedTable::zero_padding(size_t entries, hipStream_t st) {
  const size_t w = wide ? 4 : 2;
  CC_HIP(hipMemsetAsync(val.p + entries, 0, PAD * sizeof(float), st));
  CC_HIP(hipMemsetAsync(static_cast<char*>(idx()) + entries * w, 0, PAD * w, st));
  return CC_OK;
}
void SortedTable::release(size_t keep, bool wide_) {
  wide = wide_;
  if (val.n > keep) val.release();
  if (idx16.n > (wide ? 0 : keep)) idx16.release();
  if (idx32.n > (wide ? keep : 0)) idx32.release();
}

cc_status ccamd::fill_sorted_table(cc_evaluator* e, RowSorter& rows, int fb, int nf, SortedTable& t, size_t group0, cc_status (*mark)(cc_evaluator*)) {
  const int N = rows.N;
  auto note = [&]() { return mark ? mark(e) : CC_OK; };
  if (cc_status st = note(); st != CC_OK) return st;
  if (cc_status st = launch_batch(e, true, e->d_haar.p, fb, fb + nf, nullptr, N, e->d_out.p, 1, 0); st != CC_OK) return st;  // dispatches HOG
  if (cc_status st = note(); st != CC_OK) return st;
  if (cc_status st = rows.sort(nf); st != CC_OK) return st;
  if (cc_status st = note(); st != CC_OK) return st;
  with_index_type(t.wide, [&](auto ti) {
    using TI = decltype(ti);
    hipLaunchKernelGGL((k_interleave<TI>), dim3((unsigned)((N + 63) / 64), (unsigned)((nf + 63) / 64)), dim3(256), 0, e->stream.s, rows.keys_out.p,
                       rows.sorted.p, nf, N, t.val.p, static_cast<TI*>(t.idx()), group0);
  });
  CC_HIP(hipGetLastError());
  return CC_OK;
}

bool ccamd::cat_sorted_table_enabled() { return std::getenv("CCAMD_SPLIT_CAT_STREAM") == nullptr; }

// ---- what a presort costs in device memory ---------------------------------------------------
// Ordered variables: resident() for every table, split() for a head, one chunk and the winner row. Categorical (LBP):
// categorical(), with the (code, sample)-sorted table while sample numbers fit its 24 bits. u128 sums: nothing can wrap.
struct PresortCosts {
  using u128 = unsigned __int128;
  u128 N, per;     // samples; bytes of a table entry: a float and a 16- or 32-bit sample number
  bool cat_table;  // LBP keeps the sorted table of k_split_cat_sorted beside the codes
  explicit PresortCosts(size_t n) : N(n), per(4 + (wide_index(n) ? 4 : 2)), cat_table(n < ((size_t)1 << 24) && cat_sorted_table_enabled()) {}
  static size_t pad64(size_t F) { return (F + 63) / 64 * 64; }
  // variables per pass: whole groups of 64, at most 2^28 values per scratch array
  size_t pass_vars() const { return std::max<size_t>(64, (((size_t)1 << 28) / (size_t)N) / 64 * 64); }
  // all tables resident plus one pass's scratch (16 B per value, as RowSorter); without the tables' read-ahead padding
  u128 resident(size_t F) const { return (u128)pad64(F) * N * per + (u128)std::min(F, pass_vars()) * N * 16; }
  // the codes, the sorted table with its padding, and one pass's scratch (the values alone where nothing is sorted)
  u128 categorical(size_t F) const {
    return (u128)F * N + (cat_table ? (u128)pad64(F) * (N + 3 + SPLIT_CAT_PAD_RANKS) * 4 : 0) + (u128)std::min(F, pass_vars()) * N * (cat_table ? 16 : 4);
  }
  // a head of R variables (a multiple of 64) with its read-ahead padding; nothing for no head
  u128 head(size_t R) const { return R ? ((u128)R * N + SortedTable::PAD) * per : 0; }
  // one chunk of C variables: its values, sorted keys, sorted indices and iota (16 B per value, as RowSorter) and its padded table
  u128 chunk(size_t C) const { return (u128)C * N * 16 + ((u128)C * N + SortedTable::PAD) * per; }
  u128 split(size_t R, size_t C) const { return head(R) + chunk(C) + N * 8; }  // N * 8: the winner row, a float and up to 4 bytes of sample number
};
// What the evaluator holds that a new presort fills again instead of allocating ...
static size_t reused_table_bytes(const cc_evaluator* e) { return e->head.bytes() + e->d_codes.n + e->d_cat_sorted.n * 4 + e->d_out.n * 4; }
// ... and what it holds for sorted tables and, while a split presort lasts, for streaming.
static size_t held_table_bytes(const cc_evaluator* e) {
  size_t b = e->head.bytes() + e->d_codes.n + e->d_cat_sorted.n * 4;
  if (e->stream_rows)
    b += e->d_out.n * 4 + e->stream_rows->bytes() + e->chunk.bytes() + e->d_win_val.n * 4 + e->d_win_idx.n * 4 + e->d_win_state.n * sizeof(StreamBest);
  return b;
}
// `need` (a sum of PresortCosts) has to fit what is free plus what the evaluator already holds for it.
static cc_status presort_memory_check(const cc_evaluator* e, const char* who, PresortCosts::u128 need) {
  size_t free_b = 0, total_b = 0;
  CC_HIP(hipMemGetInfo(&free_b, &total_b));
  const size_t have = reused_table_bytes(e);
  if (need > (PresortCosts::u128)free_b + have)
    return set_error(CC_ERR_UNSUPPORTED, "%s: needs %.1f GB of device memory (%.1f GB free)", who, (double)need / 1e9, (double)(free_b + have) / 1e9);
  return CC_OK;
}

// Sorted values and sample numbers of the F ordered variables (Haar, HOG) from fi_begin into the resident tables, a pass at a time.
static cc_status presort_ordered(cc_evaluator* e, RowSorter& rows, int fi_begin, int F) {
  if (cc_status st = e->head.alloc(PresortCosts::pad64((size_t)F) * (size_t)rows.N, wide_index((size_t)rows.N), e->stream.s); st != CC_OK) return st;
  for (int f0 = 0; f0 < F; f0 += rows.FB)
    if (cc_status st = fill_sorted_table(e, rows, fi_begin + f0, std::min(rows.FB, F - f0), e->head, (size_t)f0 / 64, nullptr); st != CC_OK) return st;
  return CC_OK;
}

// Categorical variables (LBP): the codes [variable][sample] and, with cat_table, the (code, sample)-sorted table beside them.
static cc_status presort_categorical(cc_evaluator* e, RowSorter& rows, int fi_begin, int F, bool cat_table) {
  const int N = rows.N, FB = rows.FB;
  CC_HIP(e->d_codes.ensure((size_t)F * N));
  if (cat_table) {
    // ranks padded to a multiple of 4 per group (the tail of a group's last quad is never summed: r >= n_pre); zeroed
    // padding behind the last group for the read-ahead
    const size_t used = ((size_t)F + 63) / 64 * 64 * ((((size_t)N + 3) >> 2) << 2), pad = (size_t)SPLIT_CAT_PAD_RANKS * 64;
    CC_HIP(e->d_cat_sorted.ensure(used + pad));
    CC_HIP(hipMemsetAsync(e->d_cat_sorted.p, 0, (used + pad) * sizeof(uint32_t), e->stream.s));
  }
  for (int f0 = 0; f0 < F; f0 += FB) {
    const int f1 = std::min(F, f0 + FB), nf = f1 - f0;
    const size_t total = (size_t)nf * N;
    CC_HIP(e->d_out.ensure(total));
    if (cc_status st = launch_batch(e, false, e->d_lbp.p, fi_begin + f0, fi_begin + f1, nullptr, N, e->d_out.p, 1, 0); st != CC_OK) return st;
    hipLaunchKernelGGL(k_codes_u8, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, e->stream.s, e->d_out.p,
                       e->d_codes.p + (size_t)f0 * N, total);
    if (!cat_table) continue;
    if (cc_status st = rows.sort(nf); st != CC_OK) return st;
    hipLaunchKernelGGL(k_interleave_cat, dim3((unsigned)((N + 63) / 64), (unsigned)((nf + 63) / 64)), dim3(256), 0, e->stream.s, rows.keys_out.p,
                       rows.sorted.p, nf, N, e->d_cat_sorted.p, (size_t)f0 / 64);
  }
  CC_HIP(hipGetLastError());
  return CC_OK;
}

// ---- what the two presort entry points share: `who` is the name their messages carry ---------------------------------
static cc_status presort_check_args(const cc_evaluator* e, const char* who, int fi_begin, int fi_end, int n_samples) {
  if (!e) return set_error(CC_ERR_INVALID_ARG, "%s: null evaluator", who);
  if (n_samples < 1 || n_samples > e->max_samples)
    return set_error(CC_ERR_OUT_OF_RANGE, "%s: n_samples %d out of range (max_samples %d)", who, n_samples, e->max_samples);
  if (fi_begin < 0 || fi_end > e->nfeat || fi_begin >= fi_end)
    return set_error(CC_ERR_OUT_OF_RANGE, "%s: features [%d, %d) out of range (%d)", who, fi_begin, fi_end, e->nfeat);
  return CC_OK;
}
// The arguments are accepted: takes e->mu and, once the queued images are on the device, withdraws the tables that exist
// and gives back the chunk scratch of an earlier split presort, before anything is counted or allocated.
static cc_status presort_begin(cc_evaluator* e, std::unique_lock<std::mutex>& lk) {
  if (cc_status st = eval_device(e); st != CC_OK) return st;
  lk = std::unique_lock<std::mutex>(e->mu);
  if (cc_status st = flush_pending_images(e); st != CC_OK) return st;
  e->presort_n = 0;  // until presort_end: a failure in between leaves no tables to search
  e->generation++;   // a booster created over the earlier tables refuses its next round
  e->stream_rows.reset();
  e->chunk.release();
  e->d_win_val.release();
  e->d_win_idx.release();
  e->presort_chunk = 0;
  return CC_OK;
}
// The tables are valid: R of the range's variables resident, the others streamed C at a time (0: none are).
static cc_status presort_end(cc_evaluator* e, int fi_begin, int fi_end, int N, int cat_sorted_n, int R, int C) {
  CC_HIP(hipStreamSynchronize(e->stream.s));
  e->presort_n = N;
  e->presort_f0 = fi_begin;
  e->presort_f1 = fi_end;
  e->cat_sorted_n = cat_sorted_n;
  e->presort_resident = R;
  e->presort_chunk = C;
  return CC_OK;
}

extern "C" {

cc_status cc_eval_presort_range(cc_evaluator* e, int fi_begin, int fi_end, int n_samples) {
  if (cc_status st = presort_check_args(e, "cc_eval_presort", fi_begin, fi_end, n_samples); st != CC_OK) return st;
  std::unique_lock<std::mutex> lk;
  if (cc_status st = presort_begin(e, lk); st != CC_OK) return st;
  const bool ordered = e->type != CC_FEATURE_LBP;  // Haar and HOG
  const int F = fi_end - fi_begin, N = n_samples;
  const PresortCosts cost((size_t)N);
  const bool cat_table = !ordered && cost.cat_table;
  if (cc_status st = presort_memory_check(e, "cc_eval_presort", ordered ? cost.resident((size_t)F) : cost.categorical((size_t)F)); st != CC_OK) return st;
  RowSorter rows(e, N, (int)std::min((size_t)F, cost.pass_vars()));
  if (ordered || cat_table)
    if (cc_status st = rows.init(); st != CC_OK) return st;
  if (cc_status st = ordered ? presort_ordered(e, rows, fi_begin, F) : presort_categorical(e, rows, fi_begin, F, cat_table); st != CC_OK) return st;
  return presort_end(e, fi_begin, fi_end, N, cat_table ? N : 0, F, 0);
}

cc_status cc_eval_presort(cc_evaluator* e, int n_samples) {
  if (!e) return set_error(CC_ERR_INVALID_ARG, "cc_eval_presort: null evaluator");
  return cc_eval_presort_range(e, 0, e->nfeat, n_samples);
}

cc_status cc_eval_presort_split(cc_evaluator* e, int fi_begin, int fi_end, int n_samples, int resident_vars, int chunk_vars) {
  if (cc_status st = presort_check_args(e, "cc_eval_presort_split", fi_begin, fi_end, n_samples); st != CC_OK) return st;
  const int F = fi_end - fi_begin, N = n_samples, R = resident_vars;
  if (R == F) return cc_eval_presort_range(e, fi_begin, fi_end, n_samples);  // nothing is streamed: today's presort
  if (R < 0 || R > F || R % 64 != 0)
    return set_error(CC_ERR_INVALID_ARG, "cc_eval_presort_split: resident_vars %d is neither a multiple of 64 in [0, %d] nor %d", R, F, F);
  if (chunk_vars < 64 || chunk_vars % 64 != 0)
    return set_error(CC_ERR_INVALID_ARG, "cc_eval_presort_split: chunk_vars %d is not a multiple of 64 of at least 64", chunk_vars);
  if (e->type == CC_FEATURE_LBP)
    return set_error(CC_ERR_UNSUPPORTED, "cc_eval_presort_split: categorical variables are not streamed (LBP takes resident_vars = %d only)", F);
  std::unique_lock<std::mutex> lk;
  if (cc_status st = presort_begin(e, lk); st != CC_OK) return st;
  const PresortCosts cost((size_t)N);
  // no chunk larger than the tail or than a pass of the full presort
  const int C = (int)std::min<size_t>({(size_t)chunk_vars, PresortCosts::pad64((size_t)(F - R)), cost.pass_vars()});
  // Exactly what the plan counts is held afterwards: larger buffers of an earlier presort go back first.
  const size_t chunk_n = (size_t)C * N;
  const bool wide = wide_index((size_t)N);
  e->head.release(R ? (size_t)R * N + SortedTable::PAD : 0, wide);
  if (e->d_out.n > chunk_n) e->d_out.release();
  if (cc_status st = presort_memory_check(e, "cc_eval_presort_split", cost.split((size_t)R, (size_t)C)); st != CC_OK) return st;
  if (!e->ev_stream_a.e) CC_HIP(e->ev_stream_a.create());
  e->stream_rows.reset(new RowSorter(e, N, C));
  if (cc_status st = e->stream_rows->init(); st != CC_OK) return st;
  if (N > sort_rows_block_limit())  // the segmented sort's offsets and iota now, not inside the first node's search
    if (cc_status st = e->stream_rows->prepare_segmented(); st != CC_OK) return st;
  if (R > 0)
    if (cc_status st = presort_ordered(e, *e->stream_rows, fi_begin, R); st != CC_OK) return st;
  // a full chunk's read-ahead padding is zeroed here and never written again
  if (cc_status st = e->chunk.alloc(chunk_n, wide, e->stream.s); st != CC_OK) return st;
  CC_HIP(e->d_win_val.ensure((size_t)N));
  CC_HIP(e->d_win_idx.ensure((size_t)N));
  CC_HIP(e->d_win_state.ensure(1));
  CC_HIP(hipMemsetAsync(e->d_win_val.p, 0, (size_t)N * 4, e->stream.s));
  CC_HIP(hipMemsetAsync(e->d_win_idx.p, 0, (size_t)N * 4, e->stream.s));
  CC_HIP(hipMemsetAsync(e->d_win_state.p, 0, sizeof(StreamBest), e->stream.s));
  return presort_end(e, fi_begin, fi_end, N, 0, R, C);
}

cc_status cc_presort_plan(int feature_type, int n_vars, int n_samples, uint64_t budget_bytes, int* resident_vars, int* chunk_vars,
                          uint64_t* bytes_needed) {
  if (!resident_vars || !chunk_vars || !bytes_needed) return set_error(CC_ERR_INVALID_ARG, "cc_presort_plan: null argument");
  if (feature_type != CC_FEATURE_HAAR && feature_type != CC_FEATURE_LBP && feature_type != CC_FEATURE_HOG)
    return set_error(CC_ERR_INVALID_ARG, "cc_presort_plan: unknown feature type %d", feature_type);
  if (n_vars < 1 || n_samples < 1) return set_error(CC_ERR_OUT_OF_RANGE, "cc_presort_plan: %d variables, %d samples", n_vars, n_samples);
  *resident_vars = *chunk_vars = 0;
  *bytes_needed = 0;
  if (budget_bytes == 0) {  // what the device has free now
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
      (void)hipGetLastError();
      return set_error(CC_ERR_NO_DEVICE, "cc_presort_plan: budget_bytes = 0 asks the device for its free memory, and there is no usable HIP device");
    }
    budget_bytes = free_b;
  }
  using u128 = PresortCosts::u128;
  const size_t F = (size_t)n_vars, N = (size_t)n_samples;
  const u128 budget = budget_bytes, top = ~(uint64_t)0;
  const PresortCosts cost(N);
  auto plan = [&](size_t R, size_t C, u128 need) -> cc_status {
    *resident_vars = (int)R;
    *chunk_vars = (int)C;
    *bytes_needed = (uint64_t)need;
    return CC_OK;
  };
  if (feature_type == CC_FEATURE_LBP) {
    if (cost.categorical(F) > budget)
      return set_error(CC_ERR_UNSUPPORTED, "cc_presort_plan: categorical variables are not streamed, and their tables need %.0f bytes (budget %.0f)",
                       (double)cost.categorical(F), (double)budget);
    return plan(F, 0, cost.categorical(F));
  }
  if (cost.resident(F) <= budget) return plan(F, 0, cost.resident(F));
  if (cost.split(0, 64) > budget)
    return set_error(CC_ERR_UNSUPPORTED, "cc_presort_plan: a budget of %llu bytes holds neither every table nor one chunk of 64 variables x %d samples; the smallest budget that works is %llu",
                     (unsigned long long)budget_bytes, n_samples, (unsigned long long)std::min({cost.split(0, 64), cost.resident(F), top}));
  // Everything but the last group resident needs a chunk of 64 only (a chunk is never larger than the tail).
  const size_t r_max = (F - 1) / 64 * 64;
  if (cost.split(r_max, 64) <= budget) return plan(r_max, 64, cost.split(r_max, 64));
  // Otherwise the chunk first, up to the pass rule, and a head only beside a chunk of that size: a head that shrank
  // whenever the chunk grew by a group would not be monotone in the budget.
  const size_t c_rule = std::min(PresortCosts::pad64(F), cost.pass_vars());
  const u128 per_chunk_group = cost.chunk(128) - cost.chunk(64);  // 64 variables more
  const size_t C = (size_t)std::min<u128>(c_rule, 64 + (budget - cost.split(0, 64)) / per_chunk_group * 64);
  const u128 left = budget - cost.split(0, C), pad_bytes = cost.head(64) - (u128)64 * N * cost.per;
  const size_t R = C == c_rule && left > pad_bytes ? (size_t)std::min<u128>((left - pad_bytes) / ((u128)64 * N * cost.per) * 64, r_max) : 0;
  return plan(R, C, cost.split(R, C));
}

cc_status cc_eval_table_bytes(cc_evaluator* e, uint64_t* bytes) {
  if (!e || !bytes) return set_error(CC_ERR_INVALID_ARG, "cc_eval_table_bytes: null argument");
  std::lock_guard<std::mutex> lk(e->mu);
  *bytes = held_table_bytes(e);
  return CC_OK;
}

cc_status cc_eval_presort_budget(cc_evaluator* e, uint64_t* bytes) {
  if (!e || !bytes) return set_error(CC_ERR_INVALID_ARG, "cc_eval_presort_budget: null argument");
  if (cc_status st = eval_device(e); st != CC_OK) return st;
  std::lock_guard<std::mutex> lk(e->mu);
  size_t free_b = 0, total_b = 0;
  CC_HIP(hipMemGetInfo(&free_b, &total_b));
  *bytes = (uint64_t)free_b + held_table_bytes(e);
  return CC_OK;
}

}  // extern "C"
