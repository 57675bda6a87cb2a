// Batched, device-resident beam search of the change-captioning evaluation (reference scripts/train_CC.py:214-330, the
// loop inside `evaluate()`; decoder arithmetic of model/caption_decoder.py:316-423 and :526-613 in evaluation mode).
//
// One workgroup of 512 threads owns one image pair and runs the whole step loop itself: no grid-wide barrier, no wait on
// another workgroup, every loop bounded by max_len; a pair without a live hypothesis returns.  Per step:
//   embedding + position row of the newest token of each live hypothesis
//   per layer: qkv projection of the new row only -> K | V appended to the cache -> one-query attention over the cached
//              positions -> output projection -> LN1(x + a) -> query projection -> attention over the S memory rows of the
//              pair (projected once per pair by the caller, shared by the beams) -> output projection -> LN2(x1 + a)
//   vocabulary projection -> log-softmax (f32) -> + running score -> top-k over live x V (ties: lower flat index) ->
//   bookkeeping (parents, words, completed hypotheses, shrinking beam).
//
// Key/value cache: rows [layer][position][slot][K | V] in the workspace (L2-resident: 3 x 52 x k x 384 elements per pair).  A
// hypothesis never moves its rows: the row written at position p by slot i stays at (p, i), and every hypothesis carries the
// table anc[p] = slot that wrote ITS position p.  Reordering the beam by parent copies k small tables in LDS, not the cache.
//
// Arithmetic: f32 VALU throughout (dot products of 192 with at most 8 rows per weight row: the weights, 3 MB in f32, stream
// from L2 once per step and workgroup whatever the row count, and MFMA would leave 16 - k of its rows empty); with bf16
// activations every value the per-pair path stores in bf16 (weights in the GEMMs, qkv, attention output, projections,
// LayerNorm outputs, logits) is rounded to bf16 at the same point.  No probability matrix leaves the kernel.
#include "common.h"
#include "../../include/change3d_hip.h"

#include <climits>

namespace {

constexpr int NT = 512;        // threads per workgroup (8 waves on one CU: 1024 threads cap a thread at 128 VGPRs, which spilled)
constexpr int NW = NT / 64;
constexpr int MAXR = C3D_CAP_BEAM_MAX;   // hypotheses per pair

struct BeamLds {               // offsets in floats into the dynamic LDS region, every one a multiple of 4 (16 bytes)
  int x, x1, qkv, o, a, lg, pw, seq, anc, misc, total;
};

__host__ __device__ inline int up4(int v) { return (v + 3) & ~3; }

__host__ __device__ inline BeamLds beam_lds(int R, int D, int Vp, int S, int max_len) {
  BeamLds l;
  int o = 0;
  const int PL = up4(S > max_len ? S : max_len);
  l.x = o;    o += R * D;
  l.x1 = o;   o += R * D;
  l.qkv = o;  o += R * 3 * D;
  l.o = o;    o += R * D;
  l.a = o;    o += R * D;
  l.lg = o;   o += R * Vp;
  l.pw = o;   o += NW * PL;
  l.seq = o;  o += up4(2 * R * (max_len + 1));
  l.anc = o;  o += up4(2 * R * max_len);
  l.misc = o; o += 64 + 2 * NW + 8 * MAXR;
  l.total = up4(o);
  return l;
}

// y[r][n] = round_T(bias[n] + sum_c x[r][c] * round_T(W[n][c])) for r < rows, n < N: 8 lanes per weight row, float4 loads
// (a weight row is read once, coalesced, whatever the number of hypotheses), x rows broadcast from LDS.
template <typename T>
__device__ __forceinline__ void gemv_rows(const float* __restrict__ W, const float* __restrict__ bias, const float* xin, int ldx,
                                          float* yout, int ldy, int rows, int K, int N, int tid) {
  const int g = tid >> 3, l8 = tid & 7;
  for (int n0 = 0; n0 < N; n0 += NT / 8) {
    const int n = n0 + g;
    const bool ok = n < N;
    float acc[MAXR];
#pragma unroll
    for (int r = 0; r < MAXR; ++r) acc[r] = 0.f;
    if (ok) {
      const float* wr = W + (size_t)n * K;
#pragma unroll 2
      for (int c = l8 * 4; c < K; c += 32) {
        const float4 w4 = *reinterpret_cast<const float4*>(wr + c);
        const float w0 = round_as<T>(w4.x), w1 = round_as<T>(w4.y), w2 = round_as<T>(w4.z), w3 = round_as<T>(w4.w);
#pragma unroll
        for (int r = 0; r < MAXR; ++r)
          if (r < rows) {
            const float4 x4 = *reinterpret_cast<const float4*>(xin + r * ldx + c);
            acc[r] = fmaf(x4.x, w0, fmaf(x4.y, w1, fmaf(x4.z, w2, fmaf(x4.w, w3, acc[r]))));
          }
      }
    }
#pragma unroll
    for (int r = 0; r < MAXR; ++r) {
      float v = acc[r];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 4, 64);
      if (ok && l8 == 0 && r < rows) yout[r * ldy + n] = round_as<T>(v + bias[n]);
    }
  }
}

// y[r] = round_T(LN(x[r] + a[r])): one wave per row
template <typename T>
__device__ __forceinline__ void ln_rows(const float* x, const float* a, const float* __restrict__ gamma, const float* __restrict__ beta,
                                        float* y, int rows, int D, float eps, int tid) {
  const int wave = tid >> 6, lane = tid & 63;
  for (int r = wave; r < rows; r += NW) {
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s += x[r * D + d] + a[r * D + d];
    const float mean = wave_sum(s) / D;
    float q = 0.f;
    for (int d = lane; d < D; d += 64) { const float c = x[r * D + d] + a[r * D + d] - mean; q = fmaf(c, c, q); }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / D + eps);
    for (int d = lane; d < D; d += 64) y[r * D + d] = round_as<T>((x[r * D + d] + a[r * D + d] - mean) * rstd * gamma[d] + beta[d]);
  }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// q . k over hd elements: q in LDS (f32), k a row of T in global memory
template <typename T>
__device__ __forceinline__ float dot_row(const float* q, const T* k, int hd) {
  float s = 0.f;
  if ((hd & 7) == 0) {
    for (int d = 0; d < hd; d += 8) {
      float f[8];
      Vec8<T>::load(k + d, f);
#pragma unroll
      for (int i = 0; i < 8; ++i) s = fmaf(q[d + i], f[i], s);
    }
  } else {
    for (int d = 0; d < hd; ++d) s = fmaf(q[d], ld1<T>(k + d), s);
  }
  return s;
}

// One query row against n key/value rows: row j of K at kbase + rowoff(j), of V `voff` elements further.  pw: the wave's
// LDS scratch of >= n floats.  Result o[d] (d < hd) in lanes < hd.
template <typename T, class RowOff>
__device__ __forceinline__ float attend(const float* q, const T* kbase, int voff, int n, int hd, float* pw, int lane, RowOff rowoff) {
  float mx = -INFINITY;
  for (int j = lane; j < n; j += 64) {
    const float s = dot_row<T>(q, kbase + rowoff(j), hd);
    pw[j] = s;
    mx = fmaxf(mx, s);
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j < n; j += 64) { const float e = expf(pw[j] - mx); pw[j] = e; sum += e; }
  const float inv = 1.f / wave_sum(sum);
  for (int j = lane; j < n; j += 64) pw[j] *= inv;
  __builtin_amdgcn_wave_barrier();
  const int np = 64 / hd;
  const int part = lane / hd, d = lane - part * hd;
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f;
  if (part < np) {
    const T* vb = kbase + voff + d;
    int j = part;
    for (; j + 3 * np < n; j += 4 * np) {
      o0 = fmaf(pw[j], ld1<T>(vb + rowoff(j)), o0);
      o1 = fmaf(pw[j + np], ld1<T>(vb + rowoff(j + np)), o1);
      o2 = fmaf(pw[j + 2 * np], ld1<T>(vb + rowoff(j + 2 * np)), o2);
      o3 = fmaf(pw[j + 3 * np], ld1<T>(vb + rowoff(j + 3 * np)), o3);
    }
    for (; j < n; j += np) o0 = fmaf(pw[j], ld1<T>(vb + rowoff(j)), o0);
  }
  const float o = (o0 + o1) + (o2 + o3);
  float tot = o;
  for (int g = 1; g < np; ++g) tot += __shfl(o, d + g * hd, 64);
  __builtin_amdgcn_wave_barrier();
  return tot;
}

template <typename T>
__global__ __launch_bounds__(NT) void cap_beam_kernel(const c3d_cap_beam_args A) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int R = A.beam, D = A.D, H = A.H, hd = D / H, V = A.V, Vp = up4(V), S = A.S, B = A.B, ML = A.max_len;
  const BeamLds l = beam_lds(R, D, Vp, S, ML);
  float* xs = sm + l.x;
  float* x1s = sm + l.x1;
  float* qkv = sm + l.qkv;
  float* os = sm + l.o;
  float* as = sm + l.a;
  float* lg = sm + l.lg;
  float* pw = sm + l.pw + wave * up4(S > ML ? S : ML);
  int* seq = reinterpret_cast<int*>(sm + l.seq);      // [2][R][ML + 1]
  int* anc = reinterpret_cast<int*>(sm + l.anc);      // [2][R][ML]
  float* redv = sm + l.misc;                          // [NW]
  int* redi = reinterpret_cast<int*>(sm + l.misc + NW);          // [NW]
  float* score = sm + l.misc + 2 * NW;                // [2][MAXR] running scores
  int* selp = reinterpret_cast<int*>(score + 2 * MAXR);          // [MAXR] parent
  int* selw = selp + MAXR;                            // [MAXR] word
  float* sels = reinterpret_cast<float*>(selw + MAXR);           // [MAXR] score
  int* dest = reinterpret_cast<int*>(sels + MAXR);    // [MAXR] >= 0: new slot; < 0: -(1 + index of the completed hypothesis)
  int* st = dest + MAXR + MAXR;                       // [0] live, [1] completed so far
  const int SQ = ML + 1;
  const float scale = 1.0f / sqrtf((float)hd);
  T* cache = reinterpret_cast<T*>(A.ws) + (size_t)b * A.n_layer * ML * R * 2 * D;
  const int tstride = 1 + 3 * R;

  for (int i = tid; i < 2 * R * SQ; i += NT) seq[i] = (i % SQ) == 0 ? A.start_id : 0;
  for (int i = tid; i < 2 * R * ML; i += NT) anc[i] = 0;
  if (tid < 2 * MAXR) score[tid] = 0.f;
  if (tid == 0) { st[0] = R; st[1] = 0; }
  __syncthreads();

  int cur = 0, live = R, ncomp = 0, step = 1;
  for (; step < ML; ++step) {
    const int pos = step - 1;
    const int rows = step == 1 ? 1 : live;         // at step 1 every hypothesis is <start>: only hypothesis 0 is expanded
    const int* sq = seq + cur * R * SQ;
    int* an = anc + cur * R * ML;
    // ---- embedding + position of the newest token
    for (int i = tid; i < rows * D; i += NT) {
      const int r = i / D, d = i - r * D;
      int w = sq[r * SQ + pos];
      w = w < 0 ? 0 : (w >= V ? V - 1 : w);
      xs[i] = round_as<T>(A.emb[(size_t)w * D + d] + A.pe[(size_t)pos * D + d]);
    }
    if (tid < rows) an[tid * ML + pos] = tid;
    __syncthreads();
    for (int li = 0; li < A.n_layer; ++li) {
      const c3d_cap_beam_layer& Lw = A.layers[li];
      T* cl = cache + (size_t)li * ML * R * 2 * D;
      // ---- self-attention: qkv of the new row, K | V appended to the cache
      gemv_rows<T>(Lw.sa_in_w, Lw.sa_in_b, xs, D, qkv, 3 * D, rows, D, 3 * D, tid);
      __syncthreads();
      for (int i = tid; i < rows * 2 * D; i += NT) {
        const int r = i / (2 * D), c = i - r * 2 * D;
        st1<T>(cl + ((size_t)pos * R + r) * 2 * D + c, qkv[r * 3 * D + D + c]);
      }
      for (int i = tid; i < rows * D; i += NT) { const int r = i / D, c = i - r * D; qkv[r * 3 * D + c] *= scale; }
      __syncthreads();
      for (int t = wave; t < rows * H; t += NW) {
        const int r = t / H, h = t - r * H;
        const int* ar = an + r * ML;
        const float o = attend<T>(qkv + r * 3 * D + h * hd, cl + h * hd, D, step, hd, pw, lane,
                                  [=](int j) { return ((size_t)j * R + ar[j]) * 2 * D; });
        if (lane < hd) os[r * D + h * hd + lane] = round_as<T>(o);
      }
      __syncthreads();
      gemv_rows<T>(Lw.sa_out_w, Lw.sa_out_b, os, D, as, D, rows, D, D, tid);
      __syncthreads();
      ln_rows<T>(xs, as, Lw.n1_g, Lw.n1_b, x1s, rows, D, A.ln_eps, tid);
      __syncthreads();
      // ---- attention over the pair's memory rows (shared by the beams)
      gemv_rows<T>(Lw.ca_q_w, Lw.ca_q_b, x1s, D, qkv, 3 * D, rows, D, D, tid);
      __syncthreads();
      for (int i = tid; i < rows * D; i += NT) { const int r = i / D, c = i - r * D; qkv[r * 3 * D + c] *= scale; }
      __syncthreads();
      const T* kv = reinterpret_cast<const T*>(Lw.kv) + (size_t)b * 2 * D;
      for (int t = wave; t < rows * H; t += NW) {
        const int r = t / H, h = t - r * H;
        const float o = attend<T>(qkv + r * 3 * D + h * hd, kv + h * hd, D, S, hd, pw, lane,
                                  [=](int j) { return (size_t)j * B * 2 * D; });
        if (lane < hd) os[r * D + h * hd + lane] = round_as<T>(o);
      }
      __syncthreads();
      gemv_rows<T>(Lw.ca_out_w, Lw.ca_out_b, os, D, as, D, rows, D, D, tid);
      __syncthreads();
      ln_rows<T>(x1s, as, Lw.n2_g, Lw.n2_b, xs, rows, D, A.ln_eps, tid);
      __syncthreads();
    }
    // ---- vocabulary projection, log-softmax, running scores
    gemv_rows<T>(A.wdc_w, A.wdc_b, xs, D, lg, Vp, rows, D, V, tid);
    __syncthreads();
    if (A.logits_out)
      for (int i = tid; i < rows * V; i += NT) {
        const int r = i / V, v = i - r * V;
        A.logits_out[(((size_t)b * (ML - 1) + pos) * R + r) * V + v] = lg[r * Vp + v];
      }
    for (int r = wave; r < rows; r += NW) {
      float mx = -INFINITY;
      for (int v = lane; v < V; v += 64) mx = fmaxf(mx, lg[r * Vp + v]);
      mx = wave_max(mx);
      float sum = 0.f;
      for (int v = lane; v < V; v += 64) sum += expf(lg[r * Vp + v] - mx);
      const float lse = logf(wave_sum(sum));
      const float run = score[cur * MAXR + r];
      for (int v = lane; v < V; v += 64) lg[r * Vp + v] = run + ((lg[r * Vp + v] - mx) - lse);
    }
    __syncthreads();
    // ---- top-`live` of the rows x V candidates, in rank order; ties go to the lower flat index r * V + v
    const int ncand = rows * V;
    for (int k = 0; k < live; ++k) {
      if (A.forced) {
        if (tid == 0) {
          const int* f = A.forced + (((size_t)b * (ML - 1) + pos) * R + k) * 2;
          int p = f[0], w = f[1];
          p = p < 0 ? 0 : (p >= rows ? rows - 1 : p);
          w = w < 0 ? 0 : (w >= V ? V - 1 : w);
          selp[k] = p; selw[k] = w; sels[k] = lg[p * Vp + w];
        }
        continue;
      }
      float bv = -INFINITY;
      int bi = INT_MAX;
      for (int i = tid; i < ncand; i += NT) {
        const int r = i / V, v = i - r * V;
        const float c = lg[r * Vp + v];
        if (c > bv || (c == bv && i < bi)) { bv = c; bi = i; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
      }
      if (lane == 0) { redv[wave] = bv; redi[wave] = bi; }
      __syncthreads();
      if (tid == 0) {
        for (int w = 1; w < NW; ++w)
          if (redv[w] > bv || (redv[w] == bv && redi[w] < bi)) { bv = redv[w]; bi = redi[w]; }
        if (bi == INT_MAX) { bi = 0; bv = lg[0]; }   // nothing comparable (every candidate NaN): stay inside the table
        const int r = bi / V, v = bi - r * V;
        selp[k] = r; selw[k] = v; sels[k] = bv;
        lg[r * Vp + v] = -INFINITY;
        if (bv == -INFINITY) lg[r * Vp + v] = __int_as_float(0x7fc00000);   // an exhausted -inf candidate is not picked twice
      }
      __syncthreads();
    }
    // ---- bookkeeping: completed hypotheses leave the beam in rank order, the others become slots 0 .. k'-1
    if (tid == 0) {
      int nl = 0, nc = ncomp;
      for (int k = 0; k < live; ++k) {
        if (selw[k] == A.end_id) {
          dest[k] = -(1 + nc);
          A.comp_len[b * R + nc] = step + 1;
          A.comp_score[b * R + nc] = sels[k];
          ++nc;
        } else {
          dest[k] = nl;
          score[(cur ^ 1) * MAXR + nl] = sels[k];
          ++nl;
        }
      }
      st[0] = nl; st[1] = nc;
    }
    __syncthreads();
    if (A.trace) {
      int* tr = A.trace + ((size_t)b * (ML - 1) + pos) * tstride;
      if (tid == 0) tr[0] = live;
      if (tid < live) { tr[1 + 3 * tid] = selp[tid]; tr[2 + 3 * tid] = selw[tid]; tr[3 + 3 * tid] = __float_as_int(sels[tid]); }
    }
    {
      int* nsq = seq + (cur ^ 1) * R * SQ;
      int* nan_ = anc + (cur ^ 1) * R * ML;
      for (int i = tid; i < live * SQ; i += NT) {
        const int k = i / SQ, p = i - k * SQ;
        const int v = p < step ? sq[selp[k] * SQ + p] : (p == step ? selw[k] : 0);
        const int dk = dest[k];
        if (dk >= 0) nsq[dk * SQ + p] = v;
        else A.comp_seq[((size_t)b * R + (-dk - 1)) * SQ + p] = v;
      }
      for (int i = tid; i < live * ML; i += NT) {
        const int k = i / ML, p = i - k * ML;
        const int dk = dest[k];
        if (dk >= 0) nan_[dk * ML + p] = p < step ? an[selp[k] * ML + p] : 0;
      }
    }
    __syncthreads();
    live = st[0]; ncomp = st[1];
    cur ^= 1;
    if (live == 0) break;
  }
  // ---- the winner: FIRST maximum of the completed scores (reference :326-330); none completed: no caption
  if (tid == 0) {
    int best = -1;
    float bs = -INFINITY;
    for (int i = 0; i < ncomp; ++i) {
      const float s = A.comp_score[b * R + i];
      if (best < 0 || s > bs) { best = i; bs = s; }
    }
    int* m = A.meta + b * 4;
    m[0] = ncomp; m[1] = best; m[2] = step < ML ? step : ML - 1; m[3] = live;
  }
}

int plan(int32_t S, int32_t D, int32_t H, int32_t n_layer, int32_t V, int32_t beam, int32_t max_len, int32_t dtype, int64_t B,
         int64_t* ws_bytes, int64_t* lds_bytes) {
  if (S <= 0 || D <= 0 || H <= 0 || n_layer <= 0 || V <= 0 || beam <= 0 || max_len < 2 || B < 0) return C3D_E_BADARG;
  if (dtype != C3D_DT_F32 && dtype != C3D_DT_BF16) return C3D_E_BADARG;
  if (beam > C3D_CAP_BEAM_MAX || n_layer > C3D_CAP_BEAM_LAYERS || (D & 7) || D > 256 || D % H) return C3D_E_UNSUPPORTED;
  if (D / H > 32 || max_len > 64 || B > 65535) return C3D_E_UNSUPPORTED;
  if ((int64_t)V * beam >= (1 << 24) || S > (1 << 16)) return C3D_E_UNSUPPORTED;
  const BeamLds l = beam_lds(beam, D, up4(V), S, max_len);
  const int64_t lds = (int64_t)l.total * 4;
  if (lds > 160 * 1024) return C3D_E_UNSUPPORTED;
  if (lds_bytes) *lds_bytes = lds;
  if (ws_bytes) *ws_bytes = B * n_layer * max_len * beam * 2 * D * (dtype == C3D_DT_F32 ? 4 : 2);
  return 0;
}

}  // namespace

extern "C" int c3d_cap_beam_plan(int32_t S, int32_t D, int32_t H, int32_t n_layer, int32_t V, int32_t beam, int32_t max_len,
                                 int32_t dtype, int64_t B, int64_t* ws_bytes, int64_t* lds_bytes) {
  return plan(S, D, H, n_layer, V, beam, max_len, dtype, B, ws_bytes, lds_bytes);
}

extern "C" int c3d_cap_beam_search(const c3d_cap_beam_args* a, void* stream) {
  if (!a) return C3D_E_BADARG;
  int64_t ws = 0, lds = 0;
  const int rc = plan(a->S, a->D, a->H, a->n_layer, a->V, a->beam, a->max_len, a->dtype, a->B, &ws, &lds);
  if (rc) return rc;
  if (a->B == 0) return 0;
  if (!a->emb || !a->pe || !a->wdc_w || !a->wdc_b || !a->ws || !a->comp_seq || !a->comp_len || !a->comp_score || !a->meta)
    return C3D_E_BADARG;
  if (a->start_id < 0 || a->start_id >= a->V) return C3D_E_BADARG;
  for (int i = 0; i < a->n_layer; ++i) {
    const c3d_cap_beam_layer& L = a->layers[i];
    if (!L.sa_in_w || !L.sa_in_b || !L.sa_out_w || !L.sa_out_b || !L.n1_g || !L.n1_b || !L.ca_q_w || !L.ca_q_b || !L.ca_out_w ||
        !L.ca_out_b || !L.n2_g || !L.n2_b || !L.kv)
      return C3D_E_BADARG;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (a->dtype == C3D_DT_F32) return c3d_launch_lds<cap_beam_kernel<float>>(dim3(a->B), dim3(NT), (size_t)lds, s, *a);
  return c3d_launch_lds<cap_beam_kernel<bf16_t>>(dim3(a->B), dim3(NT), (size_t)lds, s, *a);
}
