// Caption metrics of the change-captioning validation on token ids: the BLEU-1..4 statistics, ROUGE-L and CIDEr of reference
// eval_func/bleu/bleu_scorer.py:60-83, rouge/rouge.py:23-128 and cider/cider_scorer.py:93-182, and the change / no-change
// bookkeeping of reference scripts/train_CC.py:347-376.  No strings: an n-gram of order 1..4 is one exact 64-bit key, four
// 16-bit fields holding token + 1 (0 = no token), so a key of order k has exactly k non-zero fields, keys of different orders
// never meet, and 0 is "no n-gram".  Nothing is decided by a hash: the hash only picks where a probe starts.
//
//   cap_strip_kernel            (c3d_cap_strip) one wave per raw row: drops <start> / <end> / <pad>, keeps the order (ballot +
//                               popcount), writes the compact row of 64 and its length.
//   cap_metrics_stats_kernel    one workgroup per selected image, one wave per sentence (wave 0 the hypothesis, wave 1 + r
//                               reference r); tokens and keys in LDS, every count is a compare of a lane's key against the 64
//                               keys of a sentence read as LDS broadcasts.  BLEU integers, LCS (bit-parallel, one 64-bit word),
//                               ROUGE-L, the no-change flags, and the document frequency: each n-gram that occurs first in
//                               its image's references goes once into a global open-addressing table (u64 key, u32 count).
//   cap_metrics_cider_kernel    after the table is complete (next launch on the stream): tf-idf vectors, norms, clipped
//                               cosine, length penalty; float64, every sum in ascending first-occurrence position.
//   cap_metrics_reduce_kernel   one workgroup: u64 sums of the integers, a fixed-order tree over the float64 scores.
//
// One stream, no host read in between, no grid barrier, no loop that waits for another workgroup.  Every probe loop is capped
// at the table capacity; a reached cap, a selection index outside the corpus or a malformed sentence becomes a bit of the
// status word in the totals.
#include "common.h"
#include "../../include/change3d_hip.h"

#pragma clang fp contract(off)   // the float64 expressions are the reference's, operation by operation

namespace {

typedef unsigned long long u64;

constexpr int LANES = 64;                                  // sentence positions = lanes of a wave
constexpr int WS_HEADER = 256;                             // bytes in front of the table; word 0 = status
enum { ST_TABLE_FULL = 1, ST_BAD_SELECTION = 2, ST_BAD_SENTENCE = 4 };

struct Dev {                                               // what the kernels read of c3d_cap_metrics_args
  const int32_t *hyp, *hyp_len, *refs, *ref_len, *sel, *nochange, *nochange_len;
  int32_t *stats, *lcs, *flags;
  double *rouge, *cider;
  uint32_t* status;
  u64* keys;
  uint32_t* counts;
  int32_t N, R, L, M, K, cap;
};

__device__ __forceinline__ uint32_t slot_of(u64 x, uint32_t mask) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return (uint32_t)x & mask;
}

__device__ __forceinline__ int wave_sum_i(int v) {
  for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// LDS of the two per-image kernels: tokens i32 [W][64], keys u64 [W][4][64], then the kernel's own words
__device__ __forceinline__ u64* lds_keys(char* lds, int W) { return reinterpret_cast<u64*>(lds + W * LANES * 4); }
__host__ __device__ constexpr int lds_common(int W) { return W * LANES * 4 + W * 4 * LANES * 8; }

// Wave `w` loads its sentence of image `img`; returns the length.  A length outside [0, L], a token outside [0, 65534] or an
// empty reference sets ST_BAD_SENTENCE and empties the sentence.
__device__ int load_sentence(const Dev& a, int img, int w, int lane, char* lds, int W) {
  int32_t* tok = reinterpret_cast<int32_t*>(lds) + w * LANES;
  u64* key = lds_keys(lds, W) + w * 4 * LANES;
  const int32_t* row = w == 0 ? a.hyp + (int64_t)img * a.L : a.refs + ((int64_t)img * a.R + (w - 1)) * a.L;
  int len = w == 0 ? a.hyp_len[img] : a.ref_len[(int64_t)img * a.R + (w - 1)];
  bool bad = len < 0 || len > a.L || (w > 0 && len == 0);
  if (bad) len = 0;
  int t = lane < len ? row[lane] : -1;
  if (__ballot(lane < len && (t < 0 || t > 65534))) { bad = true; len = 0; t = -1; }
  if (bad && lane == 0) atomicOr(a.status, (uint32_t)ST_BAD_SENTENCE);
  tok[lane] = t;
  u64 k = 0;
  for (int n = 0; n < 4; ++n) {                            // order n + 1
    const int tn = __shfl(t, (lane + n) & 63);
    k |= (u64)(uint32_t)(tn + 1) << (16 * n);
    key[n * LANES + lane] = lane + n < len ? k : 0ull;
  }
  return len;
}

// occurrences of `key` among the 64 keys of one (sentence, order); `first` = position of the first one, 64 if none
__device__ __forceinline__ int count_in(const u64* keys, u64 key, int& first) {
  int c = 0;
  first = LANES;
#pragma unroll 8
  for (int j = LANES - 1; j >= 0; --j) {
    const bool eq = keys[j] == key;
    c += eq;
    first = eq ? j : first;
  }
  return c;
}

// is the sentence in `tok` (length len) one of the K no-change rows?
__device__ bool is_nochange(const Dev& a, const int32_t* tok, int len, int lane) {
  bool hit = false;
  for (int k = 0; k < a.K; ++k) {
    const int nl = a.nochange_len[k];
    if (nl != len || nl < 0 || nl > a.L) continue;         // wave-uniform
    const bool differ = lane < len && a.nochange[k * a.L + lane] != tok[lane];
    if (__ballot(differ) == 0) hit = true;
  }
  return hit;
}

__device__ __forceinline__ int selected(const Dev& a, int m, bool& ok) {
  const int img = a.sel ? a.sel[m] : m;
  ok = img >= 0 && img < a.N;
  if (!ok && threadIdx.x == 0) atomicOr(a.status, (uint32_t)ST_BAD_SELECTION);
  return img;
}

__global__ __launch_bounds__(512) void cap_metrics_stats_kernel(const Dev a) {
  extern __shared__ char lds[];
  const int W = a.R + 1, lane = threadIdx.x & 63, w = threadIdx.x >> 6, m = blockIdx.x;
  int32_t* tok = reinterpret_cast<int32_t*>(lds);
  u64* keys = lds_keys(lds, W);
  int32_t* s_len = reinterpret_cast<int32_t*>(lds + lds_common(W));     // [W]
  int32_t* s_lcs = s_len + 8;                                           // [R]
  int32_t* s_flag = s_lcs + 8;                                          // [2]
  int32_t* s_correct = s_flag + 2;                                      // [4]
  bool ok;
  const int img = selected(a, m, ok);
  if (!ok) {                                               // uniform over the workgroup
    if (threadIdx.x < 10) a.stats[(int64_t)m * 10 + threadIdx.x] = 0;
    if (threadIdx.x < a.R) a.lcs[(int64_t)m * a.R + threadIdx.x] = 0;
    if (threadIdx.x == 0) { a.flags[m] = 0; a.rouge[m] = 0.0; }
    return;
  }
  const int len = load_sentence(a, img, w, lane, lds, W);
  if (lane == 0) s_len[w] = len;
  if (threadIdx.x < 2) s_flag[threadIdx.x] = 0;
  __syncthreads();

  if (w == 0) {                                            // BLEU: clipped matches of the hypothesis
    for (int n = 0; n < 4; ++n) {
      const u64 key = keys[n * LANES + lane];
      int first, f2;
      const int c_h = count_in(keys + n * LANES, key, first);
      int c_ref = 0;
      for (int r = 1; r < W; ++r) {
        const int c = count_in(keys + (r * 4 + n) * LANES, key, f2);
        c_ref = c > c_ref ? c : c_ref;
      }
      const int part = key != 0 && first == lane ? (c_h < c_ref ? c_h : c_ref) : 0;
      const int sum = wave_sum_i(part);
      if (lane == 0) s_correct[n] = sum;
    }
    if (is_nochange(a, tok, len, lane) && lane == 0) s_flag[1] = 1;
  } else {
    // document frequency: an n-gram counts once per image, at its first occurrence over the references
    const uint32_t mask = (uint32_t)a.cap - 1u;
    for (int n = 0; n < 4; ++n) {
      const u64 key = keys[(w * 4 + n) * LANES + lane];
      int first, f2;
      count_in(keys + (w * 4 + n) * LANES, key, first);
      bool fresh = key != 0 && first == lane;
      for (int r = 1; r < w; ++r) fresh = fresh && count_in(keys + (r * 4 + n) * LANES, key, f2) == 0;
      if (fresh) {
        uint32_t slot = slot_of(key, mask);
        bool done = false;
        for (int probe = 0; probe < a.cap; ++probe) {      // never waits: a slot is empty, ours, or someone else's for good
          u64 cur = __hip_atomic_load(a.keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (cur == 0) cur = atomicCAS(a.keys + slot, 0ull, key);   // a lost race returns the winner's key: compare again
          if (cur == 0 || cur == key) {
            atomicAdd(a.counts + slot, 1u);
            done = true;
            break;
          }
          slot = (slot + 1u) & mask;
        }
        if (!done) atomicOr(a.status, (uint32_t)ST_TABLE_FULL);
      }
    }
    // LCS against the hypothesis: bit i of V is clear where the LCS grows at hypothesis position i
    const int len_h = s_len[0];
    const int ht = tok[lane];
    u64 V = ~0ull;
    for (int j = 0; j < len; ++j) {
      const int rt = tok[w * LANES + j];
      const u64 Mb = __ballot(lane < len_h && ht == rt);
      V = (V + (V & Mb)) | (V & ~Mb);
    }
    if (lane == 0) s_lcs[w - 1] = __popcll(~V);
    const int flag_ref = a.R > 1 ? 1 : 0;                  // the reference looks at img_captions[1]
    if (w - 1 == flag_ref && is_nochange(a, tok + w * LANES, len, lane) && lane == 0) s_flag[0] = 1;
  }
  __syncthreads();

  if (threadIdx.x == 0) {
    const int testlen = s_len[0];
    int best_d = INT32_MAX, best_l = INT32_MAX;            // min((abs(l - testlen), l)): a tie goes to the shorter one
    double pmax = 0.0, rmax = 0.0;
    const double len_c = (double)(testlen > 0 ? testlen : 1);   // "".split(" ") is [""]: one token that matches nothing
    for (int r = 0; r < a.R; ++r) {
      const int l = s_len[r + 1], d = l > testlen ? l - testlen : testlen - l;
      if (d < best_d || (d == best_d && l < best_l)) { best_d = d; best_l = l; }
      const int c = s_lcs[r];
      a.lcs[(int64_t)m * a.R + r] = c;
      const double p = (double)c / len_c, q = l > 0 ? (double)c / (double)l : 0.0;
      pmax = p > pmax ? p : pmax;
      rmax = q > rmax ? q : rmax;
    }
    int32_t* st = a.stats + (int64_t)m * 10;
    st[0] = testlen;
    st[1] = best_l == INT32_MAX ? 0 : best_l;
    for (int n = 0; n < 4; ++n) {
      st[2 + n] = testlen - n > 0 ? testlen - n : 0;
      st[6 + n] = s_correct[n];
    }
    const double beta2 = 1.2 * 1.2;
    a.rouge[m] = pmax != 0.0 && rmax != 0.0 ? ((1.0 + beta2) * pmax * rmax) / (rmax + beta2 * pmax) : 0.0;
    a.flags[m] = s_flag[0] | (s_flag[1] << 1);
  }
}

// sum of v over the lanes in ascending lane order, the same on every lane (terms are >= 0: a lane that holds 0 changes nothing)
__device__ __forceinline__ double ordered_sum(double v) {
  double s = 0.0;
  for (int j = 0; j < LANES; ++j) s += __shfl(v, j);
  return s;
}

__global__ __launch_bounds__(512) void cap_metrics_cider_kernel(const Dev a) {
  extern __shared__ char lds[];
  const int W = a.R + 1, lane = threadIdx.x & 63, w = threadIdx.x >> 6, m = blockIdx.x;
  u64* keys = lds_keys(lds, W);
  double* vec = reinterpret_cast<double*>(lds + lds_common(W));         // [W][4][64]: tf * idf at first occurrences, else 0
  double* norm = vec + W * 4 * LANES;                                    // [W][4]
  double* val = norm + 8 * 4;                                            // [R][4]
  int32_t* s_len = reinterpret_cast<int32_t*>(val + 8 * 4);              // [W]
  bool ok;
  const int img = selected(a, m, ok);
  // a full table has lost n-grams: no score rather than a wrong one (the status says why), and no walk over a full table
  if (!ok || (*a.status & ST_TABLE_FULL)) {
    if (threadIdx.x == 0) a.cider[m] = 0.0;
    return;
  }
  const int len = load_sentence(a, img, w, lane, lds, W);
  if (lane == 0) s_len[w] = len;
  const uint32_t mask = (uint32_t)a.cap - 1u;
  const double ref_len = a.M == 1 ? 1.0 : log((double)a.M);
  for (int n = 0; n < 4; ++n) {
    const u64 key = keys[(w * 4 + n) * LANES + lane];
    int first;
    const int tf = count_in(keys + (w * 4 + n) * LANES, key, first);    // the wave reads only what it wrote itself
    double v = 0.0;
    if (key != 0 && first == lane) {
      uint32_t df = 0, slot = slot_of(key, mask);
      for (int probe = 0; probe < a.cap; ++probe) {
        const u64 cur = a.keys[slot];
        if (cur == key) { df = a.counts[slot]; break; }
        if (cur == 0) break;
        slot = (slot + 1u) & mask;
      }
      // in every selected image: idf is exactly 0, decided on the integers (one image: ref_len is 1, idf is 1 - log 1)
      const double idf = a.M > 1 && df == (uint32_t)a.M ? 0.0 : ref_len - log(df > 1 ? (double)df : 1.0);
      v = (double)tf * idf;
    }
    vec[(w * 4 + n) * LANES + lane] = v;
    const double s = ordered_sum(v * v);
    if (lane == 0) norm[w * 4 + n] = sqrt(s);
  }
  __syncthreads();

  if (w > 0) {                                             // similarity of the hypothesis to reference w - 1
    const int lh = s_len[0] > 1 ? s_len[0] - 1 : 0, lr = len > 1 ? len - 1 : 0;   // `length` counts the BIGRAMS (n == 1 is
    const double delta = (double)(lh - lr);                                       // zero-based in the reference); kept
    const double penalty = exp(-(delta * delta) / (2.0 * 6.0 * 6.0));
    for (int n = 0; n < 4; ++n) {
      const u64 key = keys[n * LANES + lane];
      const double vh = vec[n * LANES + lane];             // 0 unless this lane is a first occurrence in the hypothesis
      int first;
      count_in(keys + (w * 4 + n) * LANES, key, first);
      const double vr = key != 0 && first < LANES ? vec[(w * 4 + n) * LANES + first] : 0.0;
      double v = ordered_sum((vh < vr ? vh : vr) * vr);
      const double nh = norm[n], nr = norm[w * 4 + n];
      if (nh != 0.0 && nr != 0.0) v /= nh * nr;
      v *= penalty;
      if (lane == 0) val[(w - 1) * 4 + n] = v;
    }
  }
  __syncthreads();

  if (threadIdx.x == 0) {
    double mean = 0.0;
    for (int n = 0; n < 4; ++n) {
      double s = 0.0;
      for (int r = 0; r < a.R; ++r) s += val[r * 4 + n];
      mean += s;
    }
    mean /= 4.0;
    mean /= (double)a.R;
    a.cider[m] = mean * 10.0;
  }
}

// totals i64 [C3D_CAP_TOTALS]: 0..9 sums of the stats columns, 10 images whose flagged reference is a no-change sentence, 11
// those of them whose hypothesis is one too, 12 the other images, 13 those of them whose hypothesis is none, 14 / 15 the sums
// of rouge / cider as float64 bits, 16 the status word.
__global__ __launch_bounds__(256) void cap_metrics_reduce_kernel(const Dev a, int64_t* __restrict__ totals) {
  extern __shared__ char lds[];
  u64* s = reinterpret_cast<u64*>(lds);                    // [256]
  double* sd = reinterpret_cast<double*>(lds);
  const int t = threadIdx.x;
  u64 part[14];
  double dr = 0.0, dc = 0.0;
  for (int q = 0; q < 14; ++q) part[q] = 0;
  for (int i = t; i < a.M; i += 256) {
    for (int q = 0; q < 10; ++q) part[q] += (u64)(uint32_t)a.stats[(int64_t)i * 10 + q];
    const int f = a.flags[i];
    part[10] += (u64)(f & 1);
    part[11] += (u64)((f & 3) == 3);
    part[12] += (u64)((f & 1) == 0);
    part[13] += (u64)((f & 3) == 0);
    dr += a.rouge[i];
    dc += a.cider[i];
  }
#pragma unroll
  for (int q = 0; q < 14; ++q) {
    s[t] = part[q];
    __syncthreads();
    for (int d = 128; d; d >>= 1) {
      if (t < d) s[t] += s[t + d];
      __syncthreads();
    }
    if (t == 0) totals[q] = (int64_t)s[0];
    __syncthreads();
  }
  for (int q = 0; q < 2; ++q) {                            // the same tree every run: two runs agree bit for bit
    sd[t] = q ? dc : dr;
    __syncthreads();
    for (int d = 128; d; d >>= 1) {
      if (t < d) sd[t] += sd[t + d];
      __syncthreads();
    }
    if (t == 0) totals[14 + q] = __double_as_longlong(sd[0]);
    __syncthreads();
  }
  if (t == 0) totals[16] = (int64_t)*a.status;
}

__global__ __launch_bounds__(256) void cap_strip_kernel(const int32_t* __restrict__ raw, int64_t rows, int L_in, int start_id,
                                                        int end_id, int pad_id, int32_t* __restrict__ out,
                                                        int32_t* __restrict__ out_len) {
  const int lane = threadIdx.x & 63;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
    int kept = 0;
    for (int c = 0; c < L_in; c += LANES) {
      const int t = c + lane < L_in ? raw[row * L_in + c + lane] : pad_id;
      const bool keep = c + lane < L_in && t != start_id && t != end_id && t != pad_id;
      const u64 b = __ballot(keep);
      const int pos = kept + __popcll(b & ((1ull << lane) - 1ull));
      if (keep && pos < LANES) out[row * LANES + pos] = t;
      kept += __popcll(b);
    }
    if (lane >= kept) out[row * LANES + lane] = -1;
    if (lane == 0) out_len[row] = kept;                    // > 64: c3d_cap_metrics reports the row as a bad sentence
  }
}

bool pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

}  // namespace

extern "C" int c3d_cap_strip(const int32_t* raw, int64_t rows, int32_t L_in, int32_t start_id, int32_t end_id, int32_t pad_id,
                             int32_t* out, int32_t* out_len, void* stream) {
  if (!raw || !out || !out_len || rows < 1 || L_in < 1) return C3D_E_BADARG;
  const int64_t g = (rows + 3) / 4;
  return c3d_launch_lds<cap_strip_kernel>(dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                                          raw, rows, (int)L_in, (int)start_id, (int)end_id, (int)pad_id, out, out_len);
}

extern "C" int c3d_cap_metrics_plan(int32_t N, int32_t R, int32_t L, int64_t ref_tokens, int64_t* ws_bytes,
                                    int64_t* table_capacity) {
  if (N < 1 || R < 1 || L < 1 || !ws_bytes || !table_capacity) return C3D_E_BADARG;
  if (R > C3D_CAP_METRICS_MAX_REFS || L > LANES) return C3D_E_UNSUPPORTED;
  int64_t cap = *table_capacity;
  if (cap <= 0) {                                          // the default: at most half full with every n-gram distinct
    if (ref_tokens <= 0) ref_tokens = (int64_t)N * R * L;
    cap = 2;
    while (cap < 8 * ref_tokens) cap <<= 1;
  }
  if (!pow2(cap) || cap < 2) return C3D_E_BADARG;
  if (cap > (1ll << 30)) return C3D_E_UNSUPPORTED;
  *table_capacity = cap;
  *ws_bytes = WS_HEADER + cap * 12;
  return 0;
}

extern "C" int c3d_cap_metrics(const c3d_cap_metrics_args* p, void* stream) {
  if (!p || p->N < 1 || p->R < 1 || p->L < 1 || p->M < 1 || p->n_nochange < 0) return C3D_E_BADARG;
  if (p->R > C3D_CAP_METRICS_MAX_REFS || p->L > LANES || p->n_nochange > C3D_CAP_METRICS_MAX_NOCHANGE) return C3D_E_UNSUPPORTED;
  if (!pow2(p->table_capacity) || p->table_capacity < 2 || p->table_capacity > (1ll << 30)) return C3D_E_BADARG;
  if (!p->hyp || !p->hyp_len || !p->refs || !p->ref_len || !p->ws || !p->stats || !p->lcs || !p->flags || !p->rouge ||
      !p->cider || !p->totals || (p->n_nochange > 0 && (!p->nochange || !p->nochange_len)))
    return C3D_E_BADARG;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(p->ws);
  const int64_t cap = p->table_capacity;
  Dev a;
  a.hyp = p->hyp; a.hyp_len = p->hyp_len; a.refs = p->refs; a.ref_len = p->ref_len; a.sel = p->sel;
  a.nochange = p->nochange; a.nochange_len = p->nochange_len;
  a.stats = p->stats; a.lcs = p->lcs; a.flags = p->flags; a.rouge = p->rouge; a.cider = p->cider;
  a.status = reinterpret_cast<uint32_t*>(base);
  a.keys = reinterpret_cast<u64*>(base + WS_HEADER);
  a.counts = reinterpret_cast<uint32_t*>(base + WS_HEADER + cap * 8);
  a.N = p->N; a.R = p->R; a.L = p->L; a.M = p->M; a.K = p->n_nochange; a.cap = (int32_t)cap;
  hipError_t e = hipMemsetAsync(base, 0, (size_t)(WS_HEADER + cap * 12), st);
  if (e != hipSuccess) return (int)e;
  const int W = p->R + 1;
  int rc = c3d_launch_lds<cap_metrics_stats_kernel>(dim3((unsigned)p->M), dim3(64 * W), lds_common(W) + 32 * 4, st, a);
  if (rc) return rc;
  rc = c3d_launch_lds<cap_metrics_cider_kernel>(dim3((unsigned)p->M), dim3(64 * W),
                                                lds_common(W) + W * 4 * LANES * 8 + 64 * 8 + 8 * 4, st, a);
  if (rc) return rc;
  return c3d_launch_lds<cap_metrics_reduce_kernel>(dim3(1), dim3(256), 256 * 8, st, a, p->totals);
}
