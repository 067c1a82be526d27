// Shared-prompt decode attention (best-of-K sampling): K samples of one clip attend to ONE copy of the clip's prompt K/V plus their own
// short suffix of generated tokens.  replaces HF's _expand_inputs_for_generation (generation/utils.py, reached from model_arch.py:94-108
// with num_return_sequences = K), which repeats the prompt K times in the batch and therefore in the KV cache.
//
//   prompt cache  kp, vp [B, H, Sp, hd]       one row per clip, keys 0 .. S0-1, key_mask [B, >= S0] (1 = visible)
//   suffix cache  ks, vs [B*K, H, Tmax, hd]   one row per logical row r = b*K + j, keys 0 .. T_len-1
//   out[r]  = softmax over (prompt keys of clip r / K, then the suffix keys of row r), i.e. what egomi_attn_decode gives on the
//             physically concatenated cache of row r.  A row that sees no key gives O = 0.
//
// One 256-thread workgroup per (clip, head) serves all K queries, so a prompt K/V element is loaded once per (clip, head) and step.
//   bf16, hd 64 / 128: the K queries (padded to 32) are the N side of X = K.Q^T (32 keys x 32 queries, v_mfma_f32_32x32x16_bf16; a key's
//       A fragment is a 16-byte load from its cache row).  The query is the accumulator's lane, so the online-softmax max / sum run along
//       the 16 registers plus one lane-32 exchange, and P (bf16) is the B operand of O^T = V^T.P with no data movement (the
//       forward kernel of attention.hip does the same); V^T comes from an LDS image of the V tile through ds_read_b64_tr_b16.  The four
//       waves take the 32-key tiles round-robin and their partial (m, l, O) are merged in wave order through LDS.
//   every other (dtype, hd): the 32-key K / V tiles are staged once in LDS as fp32 and all queries read them there (VALU).
// Then, in the same launch, 8 lanes per query (hd / 8 dims each) continue the online softmax over the row's own suffix keys from
// global memory and store O.  Every sum has a fixed order that does not depend on the query's slot j: a replay is bit-equal, and
// permuting the samples of a clip permutes the output rows bit for bit.
//
// Row-table form (egomi_attn_decode_shared_rows; beam search on the split cache): K = beams per clip, and suffix key t of logical row r
// lives in PHYSICAL suffix row sfx_row[r, t] of ks, vs [n_phys, H, Tmax, hd]: a beam's suffix is the path through its ancestors' rows.
//   sfx_row [B*K, >= T_len] int32; an entry outside [0, n_phys) is a masked key (its address is clamped to row 0, its score selected away).
//   Prompt phase: the code above, unchanged (the kernels are templated on ROWS; ROWS = false is egomi_attn_decode_shared, bit for bit).
//   Suffix phase: the merged prompt state (m, l, O) of every query goes through LDS, and the workgroup's 32 eight-lane groups are dealt
//       out as NS = 32 / K slices per query: group g serves query g / NS, slice g % NS (groups >= K * NS idle).  Slice s walks the keys
//       [s * C, min((s + 1) * C, T_len)), C = ceil(T_len / NS) rounded up to 4 (consume_keys' round), so the boundaries depend on
//       (K, T_len) only.  Each lane loads its hd / 8 dims of the key / value rows it is told by the table (the table entry is one
//       broadcast load per group and key).  Slice 0 continues from the prompt state; slices >= 1 start empty, leave their (m, l, O) in
//       LDS (the prompt phase's buffers, free by then), and slice 0's group merges the ceil(T_len / C) non-empty ones in slice order and
//       stores O.  At K = 4, T_len = 160 that is 5 dependent rounds of global loads per group instead of 40.
//   Order of the sums of a row: prompt (as above), slice 0 in key order on top of it, slices 1.. each in key order from empty, merge in
//       slice order: a function of (K, S0, T_len), never of the slot j.  No atomics; a replay is bit-equal; permuting the beams of a clip
//       (queries and table rows together) permutes the output rows bit for bit.
//
// Suffix pass (egomi_attn_suffix_shared; teacher-forced scoring of given candidates): every candidate row r = b*K + j brings T queries,
// suffix positions t = 0 .. T-1, logical query row (b*K + j)*T + t, and query (j, t) is the decode query of row b*K + j at T_len = t + 1:
// the prompt of clip b, then the row's own suffix keys 0 .. t.  The kernels are templated on SFX: a workgroup per (clip, head, tile of 32
// consecutive of the clip's K*T queries) runs the prompt phase above on its 32 queries (one pass of the prompt K/V through LDS per
// workgroup), then each query's 8 lanes walk its own causal cut of the suffix with the same consume_keys rounds.  Every query slot maps
// to (query row, suffix row, T_len) through QuerySlots; with SFX = false that map is the decode one and the code is what it was.  The
// bits of query (b, j, t) are those egomi_attn_decode_shared gives it at T_len = t + 1: a function of its own data and (S0, t, hd, dtype),
// never of K, T, j, b or its neighbours in the tile.  Keys > t of the suffix row and keys >= S0 of the prompt row are never read.
#include "common.h"
#include <math.h>

namespace {

template <int DPT> struct RowState { float m, l, acc[DPT]; };

// The 32 query slots of a workgroup.  Decode (SFX = false): slot s < K is logical row b*K + s, every row at suffix length T.  Suffix
// pass (SFX = true): slot s is query q0 + s of the clip's K*T queries (j, t) = ((q0 + s) / T, (q0 + s) % T), q0 = 32 * tile; it
// reads suffix row b*K + j up to key t.  The tiles of one (clip, head) are consecutive workgroups (see block_of), so the
// workgroups in flight at any time share few prompts.  Slots >= nq are dead and clamped to the last live one (their loads stay in bounds).
template <bool SFX> struct QuerySlots {
    int nq, q0, T;
    long long qbase, sbase;
    __device__ __forceinline__ QuerySlots(int b, int K, int T_, int tile) : T(T_) {
        q0 = SFX ? 32 * tile : 0;
        nq = SFX ? (K * T - q0 < 32 ? K * T - q0 : 32) : K;
        sbase = (long long)b * K;
        qbase = SFX ? sbase * T + q0 : sbase;
    }
    __device__ __forceinline__ int clamp(int s) const { return s < nq ? s : nq - 1; }
    __device__ __forceinline__ long long qrow(int s) const { return qbase + clamp(s); }                                  // of q and out
    __device__ __forceinline__ long long srow(int s) const { return SFX ? sbase + (q0 + clamp(s)) / T : qrow(s); }       // of ks / vs
    __device__ __forceinline__ int tlen(int s) const { return SFX ? (q0 + clamp(s)) % T + 1 : T; }                       // suffix keys it sees
};
// blockIdx.x -> (clip * H + head, query tile): decode has one workgroup per (clip, head); the suffix pass numbers them tile-fastest
template <bool SFX> __device__ __forceinline__ void block_of(int K, int T, int& bh, int& tile) {
    const int ntile = SFX ? (K * T + 31) / 32 : 1;
    bh = SFX ? (int)blockIdx.x / ntile : (int)blockIdx.x;
    tile = SFX ? (int)blockIdx.x % ntile : 0;
}

// DPT (4, 8 or 16) consecutive elements -> float; p aligned to the chunk
template <typename T, int DPT> __device__ __forceinline__ void load_chunk(const T* p, float (&v)[DPT]) {
    if constexpr (DPT % 8 == 0) {
#pragma unroll
        for (int c = 0; c < DPT / 8; ++c) {
            float t[8];
            load8<T>(p + 8 * c, t);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[8 * c + j] = t[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < DPT; ++j) v[j] = Cvt<T>::ld(p + j);
    }
}

// The online softmax of one query over n keys, 4 keys per round; the 8 lanes of the query's group hold DPT dims each (qd, st.acc) and
// the same (m, l).  lk / lv(key, float[DPT]) load the group's slice of a key / value row, ok(key) is the key's visibility.
template <int DPT, typename LK, typename LV, typename OK>
__device__ __forceinline__ void consume_keys(RowState<DPT>& st, const float (&qd)[DPT], int n, LK lk, LV lv, OK ok) {
    for (int t0 = 0; t0 < n; t0 += 4) {
        float s[4];
        int kr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int key = t0 + u;
            kr[u] = key < n ? key : n - 1;
            float kv[DPT];
            lk(kr[u], kv);
            float d = 0.f;
#pragma unroll
            for (int j = 0; j < DPT; ++j) d += kv[j] * qd[j];
            d += __shfl_xor(d, 1, 64);
            d += __shfl_xor(d, 2, 64);
            d += __shfl_xor(d, 4, 64);
            s[u] = (key < n && ok(kr[u])) ? d : -INFINITY;
        }
        const float mx = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
        const float m_new = fmaxf(st.m, mx);
        const float m_safe = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = st.m == -INFINITY ? 0.f : __expf(st.m - m_safe);
        float p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] = s[u] == -INFINITY ? 0.f : __expf(s[u] - m_safe);
        st.l = st.l * alpha + ((p[0] + p[1]) + (p[2] + p[3]));
        st.m = m_new;
#pragma unroll
        for (int j = 0; j < DPT; ++j) st.acc[j] *= alpha;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float vv[DPT];
            lv(kr[u], vv);
#pragma unroll
            for (int j = 0; j < DPT; ++j) st.acc[j] += p[u] * vv[j];
        }
    }
}

// suffix keys 0 .. Tlen-1 of suffix row `srow` (from global memory), then O = acc / l -> out row `orow`
template <typename T, int HD>
__device__ __forceinline__ void suffix_and_store(RowState<HD / 8>& st, const float (&qd)[HD / 8], const T* ks, const T* vs, T* out, long long ld_o,
                                                 long long srow, long long orow, int h, int H, int Tmax, int Tlen, int sub, bool live) {
    constexpr int DPT = HD / 8;
    if (Tlen > 0) {
        const T* Ks = ks + ((srow * H + h) * (long long)Tmax) * HD + sub * DPT;
        const T* Vs = vs + ((srow * H + h) * (long long)Tmax) * HD + sub * DPT;
        consume_keys<DPT>(st, qd, Tlen,
                          [&](int key, float (&v)[DPT]) { load_chunk<T, DPT>(Ks + (long long)key * HD, v); },
                          [&](int key, float (&v)[DPT]) { load_chunk<T, DPT>(Vs + (long long)key * HD, v); },
                          [](int) { return true; });
    }
    if (live) {
        const float inv = st.l > 0.f ? 1.0f / st.l : 0.f;
        T* o = out + orow * ld_o + (long long)h * HD + sub * DPT;
#pragma unroll
        for (int j = 0; j < DPT; ++j) Cvt<T>::st(o + j, st.l > 0.f ? st.acc[j] * inv : 0.f);
    }
}

// Row-table suffix (see the header): sAcc [32][pitch], sM, sL [32] hold the prompt state of query qi at index qi on entry (written by
// other threads: the caller has synchronised).  Every thread of the workgroup calls this.
template <typename T, int HD>
__device__ __forceinline__ void suffix_rows_and_store(float* sAcc, int pitch, float* sM, float* sL, const T* q, long long ld_q, float scale,
                                                      const T* ks, const T* vs, const int* sfx_row, long long ld_row, int n_phys, T* out,
                                                      long long ld_o, int b, int K, int h, int H, int Tmax, int Tlen) {
    constexpr int DPT = HD / 8;
    const int g = threadIdx.x >> 3, sub = threadIdx.x & 7;
    const int NS = 32 / K, qi = g / NS, sl = g % NS;
    const bool live = qi < K;
    const int C = ((Tlen + NS - 1) / NS + 3) & ~3;                  // keys per slice
    const int used = C > 0 ? (Tlen + C - 1) / C : 0;                // non-empty slices
    const int t_lo = sl * C;
    const int n = !live || t_lo >= Tlen ? 0 : (Tlen - t_lo < C ? Tlen - t_lo : C);
    const long long row = (long long)b * K + (live ? qi : K - 1);
    float qd[DPT];
    load_chunk<T, DPT>(q + row * ld_q + (long long)h * HD + sub * DPT, qd);
#pragma unroll
    for (int j = 0; j < DPT; ++j) qd[j] *= scale;
    RowState<DPT> st;
    st.m = -INFINITY; st.l = 0.f;
#pragma unroll
    for (int j = 0; j < DPT; ++j) st.acc[j] = 0.f;
    if (live && sl == 0) {
        st.m = sM[qi]; st.l = sL[qi];
#pragma unroll
        for (int j = 0; j < DPT; ++j) st.acc[j] = sAcc[qi * pitch + sub * DPT + j];
    }
    __syncthreads();                                                // the prompt states have been read: the buffers now hold slices
    if (n > 0) {
        const int* tab = sfx_row + row * ld_row + t_lo;
        const long long hoff = (long long)h * Tmax + t_lo;
        auto phys = [&](int key) { const int pr = tab[key]; return pr >= 0 && pr < n_phys ? pr : -1; };
        auto at = [&](const T* base, int key) {
            const int pr = phys(key);
            return base + (((long long)(pr < 0 ? 0 : pr) * H) * Tmax + hoff + key) * HD + sub * DPT;
        };
        consume_keys<DPT>(st, qd, n,
                          [&](int key, float (&v)[DPT]) { load_chunk<T, DPT>(at(ks, key), v); },
                          [&](int key, float (&v)[DPT]) {
                              load_chunk<T, DPT>(at(vs, key), v);
                              if (phys(key) < 0) {                  // p = 0 there, and 0 * (whatever row 0 holds) must stay 0
#pragma unroll
                                  for (int j = 0; j < DPT; ++j) v[j] = 0.f;
                              }
                          },
                          [&](int key) { return phys(key) >= 0; });
    }
    if (live && sl > 0 && sl < used) {
#pragma unroll
        for (int j = 0; j < DPT; ++j) sAcc[g * pitch + sub * DPT + j] = st.acc[j];
        if (sub == 0) { sM[g] = st.m; sL[g] = st.l; }
    }
    __syncthreads();
    if (live && sl == 0) {
        for (int s = 1; s < used; ++s) {
            const float m_own = sM[g + s], l_own = sL[g + s];
            const float m_new = fmaxf(st.m, m_own);
            const float m_safe = m_new == -INFINITY ? 0.f : m_new;
            const float f_old = st.m == -INFINITY ? 0.f : __expf(st.m - m_safe);
            const float f_own = m_own == -INFINITY ? 0.f : __expf(m_own - m_safe);
#pragma unroll
            for (int j = 0; j < DPT; ++j) st.acc[j] = st.acc[j] * f_old + sAcc[(g + s) * pitch + sub * DPT + j] * f_own;
            st.l = st.l * f_old + l_own * f_own;
            st.m = m_new;
        }
        const float inv = st.l > 0.f ? 1.0f / st.l : 0.f;
        T* o = out + row * ld_o + (long long)h * HD + sub * DPT;
#pragma unroll
        for (int j = 0; j < DPT; ++j) Cvt<T>::st(o + j, st.l > 0.f ? st.acc[j] * inv : 0.f);
    }
}

// ------------------------------------------------------------------------------------------------
// VALU form: any dtype, hd 32 / 64 / 128.  Thread t: query t >> 3, dims (t & 7) * hd/8 ...
// ------------------------------------------------------------------------------------------------
template <typename T, int HD, bool ROWS, bool SFX>
__global__ __launch_bounds__(256) void attn_decode_shared_valu_kernel(const T* q, long long ld_q, const T* kp, const T* vp, const uint8_t* key_mask,
                                                                      long long ld_mask, const T* ks, const T* vs, const int* sfx_row,
                                                                      long long ld_row, int n_phys, T* out, long long ld_o, int K, int H, int Sp,
                                                                      int S0, int Tmax, int Tlen, float scale) {
    constexpr int DPT = HD / 8, CPR = HD / 8;
    __shared__ __attribute__((aligned(16))) float sK[32 * HD];
    __shared__ __attribute__((aligned(16))) float sV[32 * HD];
    __shared__ int sOk[32];
    int bh, tile;
    block_of<SFX>(K, Tlen, bh, tile);
    const int b = bh / H, h = bh % H;
    const int qq = threadIdx.x >> 3, sub = threadIdx.x & 7;
    const QuerySlots<SFX> slots(b, K, Tlen, tile);
    const bool live = qq < slots.nq;
    const long long row = slots.qrow(qq);
    float qd[DPT];
    load_chunk<T, DPT>(q + row * ld_q + (long long)h * HD + sub * DPT, qd);
#pragma unroll
    for (int j = 0; j < DPT; ++j) qd[j] *= scale;
    RowState<DPT> st;
    st.m = -INFINITY; st.l = 0.f;
#pragma unroll
    for (int j = 0; j < DPT; ++j) st.acc[j] = 0.f;
    const T* Kb = kp + (long long)bh * Sp * HD;
    const T* Vb = vp + (long long)bh * Sp * HD;
    for (int k0 = 0; k0 < S0; k0 += 32) {
        __syncthreads();                                            // the previous tile has been read
        for (int c = threadIdx.x; c < 32 * CPR; c += 256) {
            const int key = c / CPR, ch = c % CPR;
            const int kr = k0 + key < S0 ? k0 + key : S0 - 1;
            float t[8];
            load8<T>(Kb + (long long)kr * HD + ch * 8, t);
            store8<float>(sK + key * HD + ch * 8, t);
            load8<T>(Vb + (long long)kr * HD + ch * 8, t);
            store8<float>(sV + key * HD + ch * 8, t);
        }
        if (threadIdx.x < 32) {
            const int key = k0 + threadIdx.x;
            sOk[threadIdx.x] = key < S0 && (!key_mask || key_mask[(long long)b * ld_mask + key] != 0);
        }
        __syncthreads();
        const int n = S0 - k0 < 32 ? S0 - k0 : 32;
        consume_keys<DPT>(st, qd, n,
                          [&](int key, float (&v)[DPT]) { load_chunk<float, DPT>(sK + key * HD + sub * DPT, v); },
                          [&](int key, float (&v)[DPT]) { load_chunk<float, DPT>(sV + key * HD + sub * DPT, v); },
                          [&](int key) { return sOk[key] != 0; });
    }
    if constexpr (ROWS) {                                           // the prompt state of query qq -> sK [32][HD], sV [0..31] (m), [32..63] (l)
        __syncthreads();                                            // the last tile has been read
#pragma unroll
        for (int j = 0; j < DPT; ++j) sK[qq * HD + sub * DPT + j] = st.acc[j];
        if (sub == 0) { sV[qq] = st.m; sV[32 + qq] = st.l; }
        __syncthreads();
        suffix_rows_and_store<T, HD>(sK, HD, sV, sV + 32, q, ld_q, scale, ks, vs, sfx_row, ld_row, n_phys, out, ld_o, b, K, h, H, Tmax, Tlen);
    } else {
        suffix_and_store<T, HD>(st, qd, ks, vs, out, ld_o, slots.srow(qq), row, h, H, Tmax, slots.tlen(qq), sub, live);
    }
}

// ------------------------------------------------------------------------------------------------
// MFMA form: bf16, hd 64 / 128
// ------------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;
typedef __attribute__((address_space(3))) bf16x4_t lds_bf16x4;

__device__ __forceinline__ int rowmap(int reg, int half) {          // C/D row of a 32x32 accumulator register
    return (reg & 3) + 8 * (reg >> 2) + 4 * half;
}
// byte offset of 16-byte chunk ch of row `row` in a [32][HD] bf16 LDS image (the swizzle of attention.hip: row reads and transposed
// reads both free of bank conflicts)
template <int HD> __device__ __forceinline__ int swz(int row) {
    return HD == 128 ? (((row & 3) << 2) | ((row >> 2) & 3)) : ((((row >> 1) & 1) << 2) | ((row >> 2) & 3));
}
template <int HD> __device__ __forceinline__ int sw_off(int row, int ch) { return 2 * HD * row + 16 * (ch ^ swz<HD>(row)); }
// transposed fragment: 8 bf16 = column (col0 + lane&31) of rows {r0 + 4*half + 0..3, r0 + 8 + 4*half + 0..3}; every lane of the wave active
template <int HD> __device__ __forceinline__ bf16x8 lds_tr8(const char* tile, int r0, int col0, int lane) {
    const int half = lane >> 5, g = (lane >> 2) & 3, p = lane & 3;
    const int col = col0 + 16 * ((lane >> 4) & 1) + 4 * p;
    const int ch = col >> 3, within = (col & 7) * 2;
    const int ra = r0 + 4 * half + g;
    const bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(tile + sw_off<HD>(ra, ch) + within));
    const bf16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(tile + sw_off<HD>(ra + 8, ch) + within));
    bf16x8 r;
    r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
    r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
    return r;
}

template <int HD, bool ROWS, bool SFX>
__global__ __launch_bounds__(256) void attn_decode_shared_mfma_kernel(const bf16_t* q, long long ld_q, const bf16_t* kp, const bf16_t* vp,
                                                                      const uint8_t* key_mask, long long ld_mask, const bf16_t* ks,
                                                                      const bf16_t* vs, const int* sfx_row, long long ld_row, int n_phys,
                                                                      bf16_t* out, long long ld_o, int K, int H, int Sp, int S0, int Tmax,
                                                                      int Tlen, float scale) {
    constexpr int DPT = HD / 8, ND = HD / 32, NK = HD / 16, CPR = HD / 8, PITCH = HD + 1;
    __shared__ __attribute__((aligned(16))) char sV[4][32 * HD * 2];
    __shared__ float sAcc[32 * PITCH];
    __shared__ float sM[32], sL[32];
    int bh, tile;
    block_of<SFX>(K, Tlen, bh, tile);
    const int b = bh / H, h = bh % H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, half = lane >> 5;

    // Q^T as the B operand: lane (r, half) holds Q[query slot r][16c + 8 half + 0..7]; dead slots are zero columns
    const QuerySlots<SFX> slots(b, K, Tlen, tile);
    bf16x8 qf[NK];
    {
        const bf16_t* qrow = q + slots.qrow(r) * ld_q + (long long)h * HD + 8 * half;
#pragma unroll
        for (int c = 0; c < NK; ++c) {
            u32x4 d = *reinterpret_cast<const u32x4*>(qrow + 16 * c);
            if (r >= slots.nq) d = u32x4{0u, 0u, 0u, 0u};
            qf[c] = __builtin_bit_cast(bf16x8, d);
        }
    }
    const bf16_t* Kb = kp + (long long)bh * Sp * HD;
    const bf16_t* Vb = vp + (long long)bh * Sp * HD;
    f32x16 o[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[dt][i] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const int ntiles = (S0 + 31) >> 5, iters = (ntiles + 3) >> 2;
    char* tileV = sV[wave];
    for (int it = 0; it < iters; ++it) {
        const int tile = it * 4 + wave, k0 = tile * 32;
        const bool active = tile < ntiles;                          // wave-uniform
        if (active) {
#pragma unroll
            for (int j = 0; j < 32 * CPR / 64; ++j) {
                const int id = j * 64 + lane, key = id / CPR, ch = id % CPR;
                const int kr = k0 + key < S0 ? k0 + key : S0 - 1;
                const u32x4 d = *reinterpret_cast<const u32x4*>(Vb + (long long)kr * HD + ch * 8);
                *reinterpret_cast<u32x4*>(tileV + sw_off<HD>(key, ch)) = d;
            }
        }
        __syncthreads();
        if (active) {
            const int key = k0 + r;
            const int kr = key < S0 ? key : S0 - 1;
            f32x16 x;
#pragma unroll
            for (int i = 0; i < 16; ++i) x[i] = 0.f;
#pragma unroll
            for (int c = 0; c < NK; ++c) {
                const u32x4 d = *reinterpret_cast<const u32x4*>(Kb + (long long)kr * HD + 16 * c + 8 * half);
                x = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, d), qf[c], x, 0, 0, 0);
            }
            const bool okk = key < S0 && (!key_mask || key_mask[(long long)b * ld_mask + kr] != 0);
            const uint32_t vis = (uint32_t)__ballot(okk) >> (4 * half);      // bit c: key k0 + 4 half + c (lanes 0..31 vote for the tile's keys)
            float mloc = -INFINITY;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float v = (vis >> rowmap(i, 0)) & 1u ? x[i] * scale : -INFINITY;
                x[i] = v;
                mloc = fmaxf(mloc, v);
            }
            mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
            const float m_new = fmaxf(m_run, mloc);
            const float m_safe = m_new == -INFINITY ? 0.f : m_new;
            const float alpha = m_run == -INFINITY ? 0.f : __expf(m_run - m_safe);
            float lsum = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float p = x[i] == -INFINITY ? 0.f : __expf(x[i] - m_safe);
                x[i] = p;
                lsum += p;
            }
            lsum += __shfl_xor(lsum, 32, 64);
            l_run = l_run * alpha + lsum;
            m_run = m_new;
#pragma unroll
            for (int dt = 0; dt < ND; ++dt)
#pragma unroll
                for (int i = 0; i < 16; ++i) o[dt][i] *= alpha;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                bf16x8 pb;
#pragma unroll
                for (int j = 0; j < 8; ++j) pb[j] = (__bf16)x[8 * s + j];
#pragma unroll
                for (int dt = 0; dt < ND; ++dt)
                    o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lds_tr8<HD>(tileV, 16 * s, 32 * dt, lane), pb, o[dt], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // merge the four waves' partial (m, l, O^T) in wave order: sAcc[query][dim], sM / sL [query]
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
            if (w == 0) {
#pragma unroll
                for (int dt = 0; dt < ND; ++dt)
#pragma unroll
                    for (int i = 0; i < 16; ++i) sAcc[r * PITCH + 32 * dt + rowmap(i, half)] = o[dt][i];
                if (half == 0) { sM[r] = m_run; sL[r] = l_run; }
            } else {
                const float m_old = sM[r], l_old = sL[r];
                const float m_new = fmaxf(m_old, m_run);
                const float m_safe = m_new == -INFINITY ? 0.f : m_new;
                const float f_old = m_old == -INFINITY ? 0.f : __expf(m_old - m_safe);
                const float f_own = m_run == -INFINITY ? 0.f : __expf(m_run - m_safe);
#pragma unroll
                for (int dt = 0; dt < ND; ++dt)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int idx = r * PITCH + 32 * dt + rowmap(i, half);
                        sAcc[idx] = sAcc[idx] * f_old + o[dt][i] * f_own;
                    }
                __builtin_amdgcn_wave_barrier();
                if (half == 0) { sM[r] = m_new; sL[r] = l_old * f_old + l_run * f_own; }
            }
        }
        __syncthreads();
    }

    if constexpr (ROWS) {                                           // the merge loop's last barrier has published sAcc / sM / sL
        suffix_rows_and_store<bf16_t, HD>(sAcc, PITCH, sM, sL, q, ld_q, scale, ks, vs, sfx_row, ld_row, n_phys, out, ld_o, b, K, h, H, Tmax, Tlen);
        return;
    }
    // 8 lanes per query: the prompt state, then the row's own suffix
    const int qq = threadIdx.x >> 3, sub = threadIdx.x & 7;
    const bool live = qq < slots.nq;
    const long long row = slots.qrow(qq);
    RowState<DPT> st;
    st.m = sM[qq]; st.l = sL[qq];
#pragma unroll
    for (int j = 0; j < DPT; ++j) st.acc[j] = sAcc[qq * PITCH + sub * DPT + j];
    float qd[DPT];
    load_chunk<bf16_t, DPT>(q + row * ld_q + (long long)h * HD + sub * DPT, qd);
#pragma unroll
    for (int j = 0; j < DPT; ++j) qd[j] *= scale;
    suffix_and_store<bf16_t, HD>(st, qd, ks, vs, out, ld_o, slots.srow(qq), row, h, H, Tmax, slots.tlen(qq), sub, live);
}

}  // namespace

enum { FORM_OWN = 0, FORM_ROWS = 1, FORM_SUFFIX = 2 };               // egomi_attn_decode_shared, ..._rows, egomi_attn_suffix_shared

// the three entry points.  FORM_SUFFIX: T_len is T, the queries per candidate row, and the grid gains the clip's ceil(K * T / 32) tiles
static int launch_shared(int form, const void* q, int64_t ld_q, const void* kprompt, const void* vprompt, const uint8_t* key_mask,
                         int64_t ld_mask, const void* ksuffix, const void* vsuffix, const int32_t* sfx_row, int64_t ld_row, int n_phys, void* out,
                         int64_t ld_o, int B, int K, int H, int hd, int Sp, int S0, int Tmax, int T_len, float scale, int dtype,
                         egomi_stream_t stream) {
    const bool rows = form == FORM_ROWS, sfx = form == FORM_SUFFIX;
    if (!q || !kprompt || !vprompt || !out) return EGOMI_E_BADARG;
    if (T_len > 0 && (!ksuffix || !vsuffix)) return EGOMI_E_BADARG;
    if (rows && T_len > 0 && !sfx_row) return EGOMI_E_BADARG;
    if (B <= 0 || H <= 0 || K < 1 || K > 32 || S0 <= 0 || S0 > Sp || T_len < 0 || T_len > Tmax || ld_q % 8 || ld_q < (int64_t)H * hd ||
        ld_o < (int64_t)H * hd)
        return EGOMI_E_SHAPE;
    const int64_t ntile = sfx ? ((int64_t)K * T_len + 31) / 32 : 1;
    if (sfx && (T_len < 1 || (int64_t)B * H * ntile > 0x7fffffff)) return EGOMI_E_SHAPE;     // (one workgroup per (clip, head, tile))
    if (rows && T_len > 0 && (ld_row < T_len || n_phys < 1)) return EGOMI_E_SHAPE;
    if (key_mask && ld_mask < S0) return EGOMI_E_SHAPE;
    if (dtype != EGOMI_BF16 && dtype != EGOMI_F32) return EGOMI_E_BADARG;
    if (hd != 32 && hd != 64 && hd != 128) return EGOMI_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(B * H * ntile));
#define SHK(KERNEL, TT)                                                                                                            \
    EGOMI_LAUNCH((KERNEL), grid, dim3(256), 0, s, (const TT*)q, (long long)ld_q, (const TT*)kprompt, (const TT*)vprompt, key_mask,  \
                 (long long)ld_mask, (const TT*)ksuffix, (const TT*)vsuffix, (const int*)sfx_row, (long long)ld_row, n_phys, (TT*)out, \
                 (long long)ld_o, K, H, Sp, S0, Tmax, T_len, scale)
#define SHF(ROWS, SFX)                                                                         \
    if (dtype == EGOMI_BF16) {                                                                 \
        if (hd == 128) SHK((attn_decode_shared_mfma_kernel<128, ROWS, SFX>), bf16_t);          \
        else if (hd == 64) SHK((attn_decode_shared_mfma_kernel<64, ROWS, SFX>), bf16_t);       \
        else SHK((attn_decode_shared_valu_kernel<bf16_t, 32, ROWS, SFX>), bf16_t);             \
    } else {                                                                                   \
        if (hd == 128) SHK((attn_decode_shared_valu_kernel<float, 128, ROWS, SFX>), float);    \
        else if (hd == 64) SHK((attn_decode_shared_valu_kernel<float, 64, ROWS, SFX>), float); \
        else SHK((attn_decode_shared_valu_kernel<float, 32, ROWS, SFX>), float);               \
    }
    if (rows) { SHF(true, false) } else if (sfx) { SHF(false, true) } else { SHF(false, false) }
#undef SHF
#undef SHK
    return egomi_launch_status();
}

extern "C" int egomi_attn_decode_shared(const void* q, int64_t ld_q, const void* kprompt, const void* vprompt, const uint8_t* key_mask,
                                        int64_t ld_mask, const void* ksuffix, const void* vsuffix, void* out, int64_t ld_o, int B, int K, int H,
                                        int hd, int Sp, int S0, int Tmax, int T_len, float scale, int dtype, egomi_stream_t stream) {
    return launch_shared(FORM_OWN, q, ld_q, kprompt, vprompt, key_mask, ld_mask, ksuffix, vsuffix, nullptr, 0, 0, out, ld_o, B, K, H, hd, Sp, S0,
                         Tmax, T_len, scale, dtype, stream);
}

extern "C" int egomi_attn_decode_shared_rows(const void* q, int64_t ld_q, const void* kprompt, const void* vprompt, const uint8_t* key_mask,
                                             int64_t ld_mask, const void* ksuffix, const void* vsuffix, const int32_t* sfx_row, int64_t ld_row,
                                             int n_phys, void* out, int64_t ld_o, int B, int K, int H, int hd, int Sp, int S0, int Tmax,
                                             int T_len, float scale, int dtype, egomi_stream_t stream) {
    return launch_shared(FORM_ROWS, q, ld_q, kprompt, vprompt, key_mask, ld_mask, ksuffix, vsuffix, sfx_row, ld_row, n_phys, out, ld_o, B, K, H,
                         hd, Sp, S0, Tmax, T_len, scale, dtype, stream);
}

extern "C" int egomi_attn_suffix_shared(const void* q, int64_t ld_q, const void* kprompt, const void* vprompt, const uint8_t* key_mask,
                                        int64_t ld_mask, const void* ksuffix, const void* vsuffix, void* out, int64_t ld_o, int B, int K, int H,
                                        int hd, int Sp, int S0, int Tmax, int T, float scale, int dtype, egomi_stream_t stream) {
    return launch_shared(FORM_SUFFIX, q, ld_q, kprompt, vprompt, key_mask, ld_mask, ksuffix, vsuffix, nullptr, 0, 0, out, ld_o, B, K, H, hd, Sp,
                         S0, Tmax, T, scale, dtype, stream);
}
