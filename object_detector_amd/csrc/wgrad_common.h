// The one copy of what the weight-gradient kernels (conv_wgrad.hip, the streaming first-layer kernel of conv_first.hip) are
// made of: the transposing fragment read, the swizzled 256-B-row tile, the pixel cursor, the column decode and the counted
// wait of the LDS ring.  A change to the swizzle, the fragment layout or the wait arithmetic is made here.
// Included after conv_common.h (f16x8, wait_vmcnt).
#pragma once

// ---- two 4-pixel rows -> one MFMA operand ------------------------------------------------------------------------------
// ds_read_b64_tr_b16 twice: lane 4q + p of a 16-lane group supplies pixel row q, 4 channels starting at 4p, and receives
// channel l15 of 4 pixels.  lo / hi = this lane's addresses inside the 4-row blocks of pixels 8*lq .. +3 and 8*lq+4 .. +7;
// the result is channel l15 of pixels 8*lq .. 8*lq+7, a v_mfma_f32_16x16x32_f16 fragment.
__device__ __forceinline__ f16x8 od_tr_frag(const char* lo, const char* hi) {
  typedef __fp16 h4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
  const h4 a = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) h4*)lo);
  const h4 b = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) h4*)hi);
  f16x8 f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[e] = (f16)a[e];
    f[4 + e] = (f16)b[e];
  }
  return f;
}

// ---- [32 pixels][128 channels] tile, 256-B rows ------------------------------------------------------------------------
// The 16-B chunk index of row r is XORed with od_wg_swz_key(r): the transposed reads of a fragment then hit every bank once.
constexpr int OD_WG_ROWB = 256;
__device__ __forceinline__ int od_wg_swz_key(int r) { return ((r & 3) | (((r >> 3) & 1) << 2)) << 1; }

// a lane's view of such a tile: the two rows (of its 8 pixels' two 4-row blocks) it addresses in a transposed read
struct od_wg_tile_reader {
  int roff[2], rkey[2], tp;
  __device__ __forceinline__ void init(int lane) {
    const int l15 = lane & 15, lq = lane >> 4;
    tp = l15 & 3;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = 8 * lq + 4 * h + (l15 >> 2);
      roff[h] = r * OD_WG_ROWB;
      rkey[h] = od_wg_swz_key(r);
    }
  }
  __device__ __forceinline__ const char* at(const char* tile, int h, int u) const {
    return tile + roff[h] + (((u >> 1) ^ rkey[h]) * 16) + (u & 1) * 8;
  }
  // the 16 channels starting at `ch` (a multiple of 16) of this lane's 8 pixels
  __device__ __forceinline__ f16x8 frag(const char* tile, int ch) const {
    const int u = ch / 4 + tp;  // 8-byte unit inside the row (16 channels = 4 units)
    return od_tr_frag(at(tile, 0, u), at(tile, 1, u));
  }
};

// ---- pixel cursor --------------------------------------------------------------------------------------------------------
// (b, ho, wo) of the linear output pixel m; advance() moves on by a K chunk without a division (Wo >= 10 on every layer, so
// a 32-pixel step wraps at most a few rows).
struct od_wg_pixel_cursor {
  int m, b, ho, wo;
  __device__ __forceinline__ void init(int m0, int HoWo, int Wo) {
    m = m0;
    const unsigned ub = (unsigned)m0 / (unsigned)HoWo;
    const unsigned pix = (unsigned)m0 - ub * (unsigned)HoWo;
    b = (int)ub;
    ho = (int)(pix / (unsigned)Wo);
    wo = (int)(pix - (unsigned)ho * (unsigned)Wo);
  }
  __device__ __forceinline__ void advance(int step, int Ho, int Wo) {
    m += step;
    int w = wo + step, h = ho, n = b;
    while (w >= Wo) {
      w -= Wo;
      if (++h == Ho) {
        h = 0;
        ++n;
      }
    }
    wo = w, ho = h, b = n;
  }
};

// ---- column decode -------------------------------------------------------------------------------------------------------
// column j of the [Cout][k*k*Cin] gradient = (tap (dy, dx), input channel ci); a lane's 8-column group never straddles a tap
// (Cin % 8 == 0) and is all inside or all outside Ktot
struct od_wg_col {
  int dy, dx, ci;
  bool ok;
};
__device__ __forceinline__ od_wg_col od_wg_col_decode(int j, int Cin, int ks, int Ktot) {
  od_wg_col c;
  const int tap = j / Cin;
  c.ci = j - tap * Cin;
  c.dy = tap / ks;
  c.dx = tap - c.dy * ks;
  c.ok = j < Ktot;
  return c;
}

// ---- the LDS ring's wait -------------------------------------------------------------------------------------------------
// Chunks are staged NSTAGE - 1 ahead, ND LDS-DMAs per chunk per wave, strictly in chunk order.  Before chunk c of n is read:
// a counted vmcnt retires it and leaves chunks c+1 .. c+NSTAGE-2 in flight, then ONE raw s_barrier (every wave's piece of
// chunk c has landed, and chunk c-1's buffer is free for the stage that follows).
template <int ND, int NSTAGE>
__device__ __forceinline__ void od_wg_ring_wait(int c, int n) {
  static_assert(NSTAGE == 3 || NSTAGE == 4, "od_wg_ring_wait: 3 or 4 stages");
  if (NSTAGE == 4 && c + 2 < n) {
    wait_vmcnt<2 * ND>();
  } else if (c + 1 < n) {
    wait_vmcnt<ND>();
  } else {
    wait_vmcnt<0>();
  }
  __builtin_amdgcn_s_barrier();
}
