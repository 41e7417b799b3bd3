// qe_attention_bf16_stored_body.hpp -- the statements of the bf16 attention kernel on bf16 rows.  NOT a header of
// declarations: it is included INSIDE the definition of a kernel `template <int D, int MODE> __global__ void k(const AttnArgs a)`
// that has declared `constexpr bool OUT16` in front of it (false: fp32 out, attn_bf16_stored_kernel; true: `out` holds bf16
// rows behind the same pointer, each element rounded once to nearest even, attn_bf16_ctx_kernel).  Only the store at the end
// reads OUT16.  Shared as text because a shared device function changed the instructions of every fp32-out instance
// (register numbering, operand order: tools/kernel_code_diff.py), as every helper tried between attn_mfma_kernel and
// attn_bf16_kernel had.
    constexpr bool MASK = (MODE & kMask) != 0, BIAS = (MODE & kBias) != 0, CAUSAL = (MODE & kCausal) != 0;
    constexpr bool VEC4 = (MODE & kVec4) != 0;
    constexpr int HALF = D / 2;                 // dims [h*HALF, h*HALF + HALF) on lane half h
    constexpr int KS = D / 16;                  // k-steps of S^T: step s takes elements 8s .. 8s+7 of the lane's run
    constexpr int NB = (D + 31) / 32;           // 32-column blocks of O^T
    constexpr int WPB = attn_wpb(D);
    // this block / wave / lane decode is also attn_mfma_kernel's
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int lo = lane & 31, hi = lane >> 5;
    const int64_t bid = blockIdx.x;
    const int qg = (int)(bid % a.qgroups);
    const int64_t nh = bid / a.qgroups;
    const int h = (int)(nh % a.H);
    const int n = (int)(nh / a.H);
    const int q0 = (qg * WPB + wave) * 32;
    if (q0 >= a.L) return;                      // wave-uniform; no barrier in this kernel
    const int64_t E = (int64_t)a.H * a.d;
    const int64_t col = (int64_t)h * a.d;
    const uint16_t *q16 = reinterpret_cast<const uint16_t *>(a.q);      // the rows are bf16 (AttnArgs)
    const uint16_t *k16 = reinterpret_cast<const uint16_t *>(a.k);
    const uint16_t *v16 = reinterpret_cast<const uint16_t *>(a.v);

    // Q^T operand: fragment s holds bf16(fp32(q[query q0 + lo][hi*HALF + 8s + j]) * scale); rows beyond L are zero
    bf16x8 qf[KS];
    {
        const int t = q0 + lo;
        const uint4 *src = reinterpret_cast<const uint4 *>(q16 + (n * a.q_rn + min(t, a.L - 1) * a.q_rt) * E + col + hi * HALF);
        const float sc = a.scale;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const uint4 x = src[s];
            qf[s] = t < a.L ? pack8(bf_lo(x.x) * sc, bf_hi(x.x) * sc, bf_lo(x.y) * sc, bf_hi(x.y) * sc, bf_lo(x.z) * sc,
                                    bf_hi(x.z) * sc, bf_lo(x.w) * sc, bf_hi(x.w) * sc)
                            : pack8(0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
    const uint16_t *kbase = k16 + n * a.kv_rn * E + col;
    const uint16_t *vbase = v16 + n * a.kv_rn * E + col;
    const int64_t kv_step = a.kv_rt * E;

    // additive operands of a tile, in the score accumulator's own order: ar[r] belongs to key crow(r, hi) of query q0 + lo
    const float *mrow = nullptr, *brow = nullptr;
    if constexpr (MASK) mrow = a.mask + n * a.mask_sn + h * a.mask_sh + (int64_t)(q0 + lo < a.L ? q0 + lo : 0) * a.S;
    if constexpr (BIAS) brow = a.key_bias + (int64_t)n * a.S;
    float ar[(MASK || BIAS) ? 16 : 1];
    // as the V loads below: every lane loads from a clamped, valid address and a select zeroes what lies beyond S
    auto load_add = [&](int k0) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int key = k0 + 8 * g + 4 * hi;
            if constexpr (VEC4) {                   // S % 4 == 0: a run lies wholly below S or wholly beyond it
                const int kc = min(key, a.S - 4);
                float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if constexpr (MASK) x = *reinterpret_cast<const float4 *>(mrow + kc);
                if constexpr (BIAS) {
                    const float4 y = *reinterpret_cast<const float4 *>(brow + kc);
                    if constexpr (MASK) { x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w; } else x = y;
                }
                const bool in = key < a.S;
                ar[4 * g] = in ? x.x : 0.0f; ar[4 * g + 1] = in ? x.y : 0.0f; ar[4 * g + 2] = in ? x.z : 0.0f;
                ar[4 * g + 3] = in ? x.w : 0.0f;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int kc = min(key + j, a.S - 1);
                    float x = 0.0f;
                    if constexpr (MASK) x = mrow[kc];
                    if constexpr (BIAS) { if constexpr (MASK) x += brow[kc]; else x = brow[kc]; }
                    ar[4 * g + j] = key + j < a.S ? x : 0.0f;
                }
            }
        }
    };
    // causal: the last tile that holds a key <= q0 + 31 is the wave's diagonal tile; the tiles above it are not visited
    const int kend = CAUSAL ? min(a.S, q0 + 32) : a.S;

    // K of the next tile waits as MFMA fragments (the loads stay in flight over the softmax): fragment s of key k0 + lo is
    // elements hi*HALF + 8s .. + 7 of its row, zero beyond S
    uint4 kr[KS];
    auto load_k = [&](int k0) {
        if constexpr (MASK || BIAS) load_add(k0);
        const int key = k0 + lo;
        const uint4 *src = reinterpret_cast<const uint4 *>(kbase + min(key, a.S - 1) * kv_step + hi * HALF);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const uint4 x = src[s];
            kr[s] = key < a.S ? x : make_uint4(0u, 0u, 0u, 0u);
        }
    };

    f32x16 o[NB];                               // zeroed as in attn_mfma_kernel
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[b][r] = 0.0f;
    float m = -INFINITY, lsum = 0.0f;

    load_k(0);
    for (int k0 = 0; k0 < kend; k0 += 32) {
        // V^T operand of this tile: register vr[i][b] holds elements 2 i (low half) and 2 i + 1 (high half) of the fragments,
        // v[key k0 + crow(2 i, hi)][32 b + lo] and the same column of the next key.  Every lane loads from a clamped, valid
        // address (key S - 1, column D - 1) and one mask per register zeroes the tail: 16 NB loads in flight together,
        // where a load under a per-lane condition becomes a branch with its own wait
        uint32_t vr[8][NB];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int key = k0 + (2 * i & 3) + 8 * (i >> 1) + 4 * hi;       // crow(2 i, hi); crow(2 i + 1, hi) is key + 1
            const uint16_t *src0 = vbase + min(key, a.S - 1) * kv_step, *src1 = vbase + min(key + 1, a.S - 1) * kv_step;
            const uint32_t keep = key + 1 < a.S ? 0xffffffffu : key < a.S ? 0xffffu : 0u;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int c = 32 * b + lo;
                const int cc = 32 * b + 31 < D ? c : min(c, D - 1);
                u16x2 w;
                w.x = src0[cc];
                w.y = src1[cc];
                vr[i][b] = __builtin_bit_cast(uint32_t, w) & (c < D ? keep : 0u);
            }
        }
        f32x16 sc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = 0.0f;
#pragma unroll
        for (int s = 0; s < KS; ++s) sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kr[s]), qf[s], sc, 0, 0, 0);
        if constexpr (MASK || BIAS) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[r] += ar[r];
        }
        if (k0 + 32 < kend) load_k(k0 + 32);

        // online softmax over this tile's 32 keys of query q0 + lo; also attn_mfma_kernel's
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (key >= a.S) sc[r] = -INFINITY;
            if constexpr (CAUSAL) { if (key > q0 + lo) sc[r] = -INFINITY; }
            tmax = fmaxf(tmax, sc[r]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float mn = fmaxf(m, tmax);
        float alpha = exp2f((m - mn) * kLog2e);
        float msub = mn;
        if constexpr (MASK || BIAS) {              // every key so far masked: -inf - -inf is NaN; keep the empty state
            if (mn == -INFINITY) { alpha = 1.0f; msub = 0.0f; }
        }
        m = mn;
        float psum = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            sc[r] = exp2f((sc[r] - msub) * kLog2e);
            psum += sc[r];
        }
        lsum = lsum * alpha + psum;
        // P^T operand: registers 8s .. 8s+7 of the score accumulator are the B fragment of k-step s
        bf16x8 pf[2];
#pragma unroll
        for (int s = 0; s < 2; ++s)
            pf[s] = pack8(sc[8 * s], sc[8 * s + 1], sc[8 * s + 2], sc[8 * s + 3], sc[8 * s + 4], sc[8 * s + 5], sc[8 * s + 6],
                          sc[8 * s + 7]);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
#pragma unroll
            for (int r = 0; r < 16; ++r) o[b][r] *= alpha;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                // elements 2i, 2i + 1 of the A fragment share a register: low and high half
                const uint4 vf = make_uint4(vr[4 * s][b], vr[4 * s + 1][b], vr[4 * s + 2][b], vr[4 * s + 3][b]);
                o[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vf), pf[s], o[b], 0, 0, 0);
            }
        }
    }

    const int t = q0 + lo;
    const float l = lsum + __shfl_xor(lsum, 32);
    if (t >= a.L) return;
    if constexpr (OUT16) {
        // the same four quotients, rounded to bf16 (v_cvt_pk_bf16_f32: nearest even, a NaN stays a NaN): one 8-byte piece
        uint16_t *dst = reinterpret_cast<uint16_t *>(a.out) + (n * a.o_rn + t * a.o_rt) * E + col;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = 32 * b + 8 * g + 4 * hi;
                if (c < D) {
                    bf16x4 w;
                    w[0] = (__bf16)(o[b][4 * g] / l); w[1] = (__bf16)(o[b][4 * g + 1] / l);
                    w[2] = (__bf16)(o[b][4 * g + 2] / l); w[3] = (__bf16)(o[b][4 * g + 3] / l);
                    *reinterpret_cast<uint2 *>(dst + c) = __builtin_bit_cast(uint2, w);
                }
            }
        }
        return;
    }
    float *dst = a.out + (n * a.o_rn + t * a.o_rt) * E + col;      // from the row-sum exchange on, also attn_mfma_kernel's
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = 32 * b + 8 * g + 4 * hi;       // O^T rows (r&3) + 8(r>>2) + 4 hi of register r = 4 g + j
            if (c < D)
                *reinterpret_cast<float4 *>(dst + c) =
                    make_float4(o[b][4 * g] / l, o[b][4 * g + 1] / l, o[b][4 * g + 2] / l, o[b][4 * g + 3] / l);
        }
    }
