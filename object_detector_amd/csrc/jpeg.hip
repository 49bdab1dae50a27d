// K15: image decode + resize into the network input (ObjectDetector(image_decode="device")).  Integer arithmetic only;
// every stage reproduces what the host path (PIL over libjpeg-turbo, then Image.resize(BILINEAR)) computes, so the
// network input is byte-identical.
//   od_jpeg_huff_k   entropy decode, one workgroup per image: the self-synchronising parallel Huffman decode of
//                    Weissenberger & Schmidt (HiPC 2021).  Subsequence j starts at a guessed state; rounds separated by
//                    barriers restart j from j-1's exit state until no exit changes; a segmented scan over block counts
//                    and DC differences places every subsequence; a last pass writes the quantised coefficients.
//   od_jpeg_idct_k   libjpeg jpeg_idct_islow (CONST_BITS 13, PASS1_BITS 2, its range limit), one thread per block
//   od_jpeg_color_k  libjpeg-turbo's default upsampling (fancy h2v1 / h2v2, replication for chroma <= 2 wide) and
//                    jdcolor's YCbCr->RGB tables (SCALEBITS 16)
//   od_img_hpass_k / od_img_vpass_k   Pillow's fixed-point BILINEAR passes (22 fraction bits; resample_common.h), letterbox zeros;
//                    horizontal then vertical, the other way round where Image.resize does so (vertical_first)
// Bounds: every stream read is clipped to its restart interval, every coefficient write to the interval's blocks, and
// the host checks every offset of the descriptors against the blob and workspace sizes before a launch.
#include "resample_common.h"

namespace {

constexpr int HT = 512;  // threads of the entropy-decode workgroup
constexpr int LOOK = 9;

__constant__ int8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct BitReader {
  const uint8_t* s;
  int end;   // bytes at or past `end` read as zero (libjpeg inserts zeros at a marker)
  int byte;  // next byte to load
  int nbits;
  uint64_t acc;  // valid bits left-aligned
  __device__ void init(const uint8_t* src, int end_byte, uint32_t pos) {
    s = src;
    end = end_byte;
    byte = (int)(pos >> 3);
    nbits = 0;
    acc = 0;
    fill();
    drop(pos & 7);
  }
  __device__ void fill() {
    while (nbits <= 56) {
      const uint64_t b = (byte >= 0 && byte < end) ? s[byte] : 0;
      acc |= b << (56 - nbits);
      nbits += 8;
      ++byte;
    }
  }
  __device__ uint32_t peek(int n) const { return (uint32_t)(acc >> (64 - n)); }
  __device__ void drop(int n) {
    acc <<= n;
    nbits -= n;
  }
  __device__ int get(int n) {
    if (n == 0) return 0;
    const int v = (int)peek(n);
    drop(n);
    return v;
  }
  __device__ uint32_t pos() const { return (uint32_t)(byte * 8 - nbits); }
};

__device__ __forceinline__ int huff(const int* t, BitReader& br) {
  const int e = t[br.peek(LOOK)];
  if (e >> 8) {
    br.drop(e >> 8);
    return e & 255;
  }
  const int code = (int)br.peek(16);
  for (int l = LOOK + 1; l <= 16; ++l) {
    const int c = code >> (16 - l);
    if (c <= t[512 + l]) {
      br.drop(l);
      return t[548 + ((c + t[530 + l]) & 255)];
    }
  }
  br.drop(16);  // corrupt data: libjpeg fakes a zero
  return 0;
}

__device__ __forceinline__ int extend(int r, int s) { return r < (1 << (s - 1)) ? r - (1 << s) + 1 : r; }

__device__ __forceinline__ uint64_t pack_state(uint32_t pos, int c, int k) {
  return (uint64_t)pos | ((uint64_t)c << 32) | ((uint64_t)k << 40);
}

// Decode the symbols of one subsequence that start before its end bit, from state `st` (bit position, block of the
// MCU, zig-zag index).  Counting mode: cnt / dc[] sum the blocks started and their DC differences.  WRITE mode: dc[]
// enters as the DC predictors and coefficients of blocks [first, end) are written.  Returns the exit state.
template <bool WRITE>
__device__ uint64_t run_sub(const uint8_t* stream, int stream_bytes, const int* sub, uint64_t st,
                            const int (*tab)[OD_JPEG_HUFF_INTS], int bpm, int luma_blocks, int& cnt, int* dc,
                            int16_t* coef, int base, int n_blocks) {
  BitReader br;
  br.init(stream, min(sub[2] >> 3, stream_bytes), (uint32_t)st);
  int c = (int)((st >> 32) & 7), k = (int)((st >> 40) & 127);
  if (c >= bpm) c = 0;
  if (k > 63) k = 0;
  const uint32_t end_bit = (uint32_t)sub[1];
  const int fb = max(sub[3], 0), eb = min(sub[4], n_blocks);
  int cur = base - 1;
  while (br.pos() < end_bit) {
    br.fill();
    const int ci = c < luma_blocks ? 0 : c - luma_blocks + 1;
    if (k == 0) {
      if (WRITE && cur + 1 >= eb) break;  // the interval's blocks are all decoded
      const int n = huff(tab[2 * ci], br);
      const int diff = n ? extend(br.get(n), n) : 0;
      ++cnt;
      dc[ci] += diff;
      if (WRITE) {
        ++cur;
        if (cur >= fb) coef[(int64_t)cur * 64] = (int16_t)dc[ci];
      }
      k = 1;
    } else {
      const int rs = huff(tab[2 * ci + 1], br);
      const int r = rs >> 4, n = rs & 15;
      if (n) {
        k += r;
        const int v = extend(br.get(n), n);
        if (WRITE && cur >= fb && cur < eb) coef[(int64_t)cur * 64 + kNatural[min(k, 63)]] = (int16_t)v;
        ++k;
      } else if (r == 15) {
        k += 16;
      } else {
        k = 64;
      }
    }
    if (k >= 64) {
      k = 0;
      if (++c == bpm) c = 0;
    }
  }
  return pack_state(br.pos(), c, k);
}

// Workspace of one image's sync state (od_img_workspace_plan sizes it): int32 header[4] (0: sync rounds), then
// u64 exit[2][n], int changed[2][n], int cnt[n], int dc[3][n]  (cnt / dc become exclusive segmented prefixes)
__global__ __launch_bounds__(HT) void od_jpeg_huff_k(const uint8_t* __restrict__ blob, const od_img_desc* __restrict__ descs,
                                                     uint8_t* __restrict__ ws) {
  const od_img_desc d = descs[blockIdx.x];
  if (d.kind != OD_IMG_JPEG) return;
  __shared__ int tab[6][OD_JPEG_HUFF_INTS];
  __shared__ int s_any;
  __shared__ int s_f[HT], s_v[4][HT];
  const int tid = threadIdx.x;
  const int* gt = (const int*)(blob + d.huff_off);
  for (int i = tid; i < 6 * OD_JPEG_HUFF_INTS; i += HT) (&tab[0][0])[i] = gt[i];
  const int luma_blocks = d.ncomp == 1 ? 1 : d.samp_h * d.samp_v;
  const int bpm = d.ncomp == 1 ? 1 : luma_blocks + 2;
  const int n_blocks = d.mcux * d.mcuy * bpm;
  int16_t* coef = (int16_t*)(ws + d.coef_ws);
  {
    int4* z = (int4*)coef;
    for (int i = tid; i < n_blocks * 8; i += HT) z[i] = make_int4(0, 0, 0, 0);
  }
  const int n = d.n_sub;
  const int* subs = (const int*)(blob + d.sub_off);
  const uint8_t* stream = blob + d.stream_off;
  const int sbytes = (int)d.stream_bytes;
  int* hdr = (int*)(ws + d.state_ws);
  uint64_t* ex[2] = {(uint64_t*)(hdr + 4), (uint64_t*)(hdr + 4) + n};
  int* ch[2] = {(int*)(ex[1] + n), (int*)(ex[1] + n) + n};
  int* cnt = ch[1] + n;
  int* dcs = cnt + n;  // [3][n]
  __syncthreads();
  // round 0: every subsequence from its own start bit, guessing "first coefficient of the MCU's first block"
  for (int j = tid; j < n; j += HT) {
    const int* sb = subs + j * OD_JPEG_SUB_INTS;
    int cn = 0, dc[3] = {0, 0, 0};
    ex[0][j] = run_sub<false>(stream, sbytes, sb, pack_state((uint32_t)sb[0], 0, 0), tab, bpm, luma_blocks, cn, dc,
                              nullptr, 0, n_blocks);
    ch[0][j] = 1;
    cnt[j] = cn;
    dcs[j] = dc[0];
    dcs[n + j] = dc[1];
    dcs[2 * n + j] = dc[2];
  }
  int cur = 0, rounds = 1;
  for (; rounds <= n + 1; ++rounds) {
    __syncthreads();
    if (tid == 0) s_any = 0;
    __syncthreads();
    const int nxt = cur ^ 1;
    for (int j = tid; j < n; j += HT) {
      const int* sb = subs + j * OD_JPEG_SUB_INTS;
      if (!sb[5] && ch[cur][j - 1]) {  // the predecessor's exit moved: restart from it
        int cn = 0, dc[3] = {0, 0, 0};
        const uint64_t e = run_sub<false>(stream, sbytes, sb, ex[cur][j - 1], tab, bpm, luma_blocks, cn, dc, nullptr, 0,
                                          n_blocks);
        cnt[j] = cn;
        dcs[j] = dc[0];
        dcs[n + j] = dc[1];
        dcs[2 * n + j] = dc[2];
        const int moved = e != ex[cur][j];
        ex[nxt][j] = e;
        ch[nxt][j] = moved;
        if (moved) s_any = 1;
      } else {
        ex[nxt][j] = ex[cur][j];
        ch[nxt][j] = 0;
      }
    }
    __syncthreads();
    cur = nxt;
    if (!s_any) break;
  }
  if (tid == 0) hdr[0] = rounds;
  // segmented exclusive scan (reset at each restart interval's first subsequence) of cnt and dc[3]: a contiguous chunk
  // per thread, then a Hillis-Steele scan of the chunk aggregates
  const int per = (n + HT - 1) / HT;
  const int j0 = min(tid * per, n), j1 = min(j0 + per, n);
  int f = 0, v[4] = {0, 0, 0, 0};
  for (int j = j0; j < j1; ++j) {
    if (subs[j * OD_JPEG_SUB_INTS + 5]) {
      f = 1;
      v[0] = v[1] = v[2] = v[3] = 0;
    }
    v[0] += cnt[j];
    v[1] += dcs[j];
    v[2] += dcs[n + j];
    v[3] += dcs[2 * n + j];
  }
  s_f[tid] = f;
  for (int q = 0; q < 4; ++q) s_v[q][tid] = v[q];
  __syncthreads();
  for (int off = 1; off < HT; off <<= 1) {
    int pf = 0, pv[4] = {0, 0, 0, 0};
    const bool has = tid >= off;
    if (has) {
      pf = s_f[tid - off];
      for (int q = 0; q < 4; ++q) pv[q] = s_v[q][tid - off];
    }
    __syncthreads();
    if (has && !s_f[tid]) {
      for (int q = 0; q < 4; ++q) s_v[q][tid] += pv[q];
      s_f[tid] = pf;
    }
    __syncthreads();
  }
  int run[4] = {0, 0, 0, 0};
  if (tid > 0)
    for (int q = 0; q < 4; ++q) run[q] = s_v[q][tid - 1];
  for (int j = j0; j < j1; ++j) {
    if (subs[j * OD_JPEG_SUB_INTS + 5]) run[0] = run[1] = run[2] = run[3] = 0;
    const int c0 = cnt[j], d0 = dcs[j], d1 = dcs[n + j], d2 = dcs[2 * n + j];
    cnt[j] = run[0];
    dcs[j] = run[1];
    dcs[n + j] = run[2];
    dcs[2 * n + j] = run[3];
    run[0] += c0;
    run[1] += d0;
    run[2] += d1;
    run[3] += d2;
  }
  __syncthreads();
  // write pass: every subsequence from its synchronised start state
  for (int j = tid; j < n; j += HT) {
    const int* sb = subs + j * OD_JPEG_SUB_INTS;
    const uint64_t st = sb[5] ? pack_state((uint32_t)sb[0], 0, 0) : ex[cur][j - 1];
    int cn = 0, dc[3] = {dcs[j], dcs[n + j], dcs[2 * n + j]};
    run_sub<true>(stream, sbytes, sb, st, tab, bpm, luma_blocks, cn, dc, coef, sb[3] + cnt[j], n_blocks);
  }
}

// libjpeg jidctint.c: one 8-point pass; `sh` = the pass's descale
__device__ __forceinline__ void idct8(int64_t x0, int64_t x1, int64_t x2, int64_t x3, int64_t x4, int64_t x5, int64_t x6,
                                      int64_t x7, int sh, int64_t* o) {
  int64_t z1 = (x2 + x6) * 4433;
  const int64_t t2 = z1 - x6 * 15137, t3 = z1 + x2 * 6270;
  const int64_t t0 = (x0 + x4) * 8192, t1 = (x0 - x4) * 8192;
  const int64_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  z1 = x7 + x1;
  int64_t z2 = x5 + x3, z3 = x7 + x3, z4 = x5 + x1;
  const int64_t z5 = (z3 + z4) * 9633;
  int64_t o0 = x7 * 2446, o1 = x5 * 16819, o2 = x3 * 25172, o3 = x1 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  o0 += z1 + z3;
  o1 += z2 + z4;
  o2 += z2 + z3;
  o3 += z1 + z4;
  const int64_t r = (int64_t)1 << (sh - 1);
  o[0] = (t10 + o3 + r) >> sh;
  o[7] = (t10 - o3 + r) >> sh;
  o[1] = (t11 + o2 + r) >> sh;
  o[6] = (t11 - o2 + r) >> sh;
  o[2] = (t12 + o1 + r) >> sh;
  o[5] = (t12 - o1 + r) >> sh;
  o[3] = (t13 + o0 + r) >> sh;
  o[4] = (t13 - o0 + r) >> sh;
}

__device__ __forceinline__ uint32_t range_limit(int64_t v) {
  int i = (int)(v & 1023);
  i = i < 512 ? i : i - 1024;
  return (uint32_t)min(max(i + 128, 0), 255);
}

// component planes of one image: plane c is (mcux*h_c*8) x (mcuy*v_c*8) bytes, planes back to back from plane_ws
__device__ __forceinline__ int64_t plane_bytes(const od_img_desc& d, int c) {
  const int hs = (c == 0 && d.ncomp == 3) ? d.samp_h : 1, vs = (c == 0 && d.ncomp == 3) ? d.samp_v : 1;
  return (int64_t)d.mcux * hs * 8 * d.mcuy * vs * 8;
}

__global__ __launch_bounds__(256) void od_jpeg_idct_k(const uint8_t* __restrict__ blob, const od_img_desc* __restrict__ descs,
                                                      uint8_t* __restrict__ ws) {
  const od_img_desc d = descs[blockIdx.y];
  if (d.kind != OD_IMG_JPEG) return;
  const int luma_blocks = d.ncomp == 1 ? 1 : d.samp_h * d.samp_v;
  const int bpm = d.ncomp == 1 ? 1 : luma_blocks + 2;
  const int n_blocks = d.mcux * d.mcuy * bpm;
  const int16_t* coef = (const int16_t*)(ws + d.coef_ws);
  const int* quant = (const int*)(blob + d.quant_off);
  for (int g = blockIdx.x * 256 + threadIdx.x; g < n_blocks; g += gridDim.x * 256) {
    const int m = g / bpm, b = g - m * bpm;
    const int ci = b < luma_blocks ? 0 : b - luma_blocks + 1;
    const int hs = ci == 0 ? (d.ncomp == 1 ? 1 : d.samp_h) : 1, vs = ci == 0 ? (d.ncomp == 1 ? 1 : d.samp_v) : 1;
    const int bx = ci == 0 ? b % hs : 0, by = ci == 0 ? b / hs : 0;
    const int mx = m % d.mcux, my = m / d.mcux;
    const int X = mx * hs + bx, Y = my * vs + by;
    const int pw = d.mcux * hs * 8;
    int64_t off = d.plane_ws;
    for (int c = 0; c < ci; ++c) off += plane_bytes(d, c);
    uint8_t* dst = ws + off + (int64_t)Y * 8 * pw + X * 8;
    int32_t x[64];
    const int4* src = (const int4*)(coef + (int64_t)g * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int4 v = src[i];
      const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        x[i * 8 + 2 * h] = (int16_t)(w[h] & 0xFFFF);
        x[i * 8 + 2 * h + 1] = (int16_t)((uint32_t)w[h] >> 16);
      }
    }
#pragma unroll
    for (int i = 0; i < 64; ++i) x[i] *= quant[ci * 64 + i];
    int32_t wsp[64];
#pragma unroll
    for (int col = 0; col < 8; ++col) {
      int64_t o[8];
      idct8(x[col], x[8 + col], x[16 + col], x[24 + col], x[32 + col], x[40 + col], x[48 + col], x[56 + col], 11, o);
#pragma unroll
      for (int r = 0; r < 8; ++r) wsp[r * 8 + col] = (int32_t)o[r];
    }
#pragma unroll
    for (int row = 0; row < 8; ++row) {
      int64_t o[8];
      const int32_t* w = wsp + row * 8;
      idct8(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], 18, o);
      uint32_t lo = 0, hi = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        lo |= range_limit(o[c]) << (8 * c);
        hi |= range_limit(o[c + 4]) << (8 * c);
      }
      *(uint2*)(dst + (int64_t)row * pw) = make_uint2(lo, hi);
    }
  }
}

// one chroma sample of the upsampled plane at full-resolution (x, y): libjpeg-turbo jdsample.c
__device__ __forceinline__ int chroma(const uint8_t* p, int pw, int cw, int ch, int hs, int vs, int x, int y) {
  if (hs == 1 && vs == 1) return p[(int64_t)y * pw + x];
  if (hs == 1) {  // h1v2 fancy
    const int i = y >> 1, nb = (y & 1) ? min(i + 1, ch - 1) : max(i - 1, 0);
    return (3 * p[(int64_t)i * pw + x] + p[(int64_t)nb * pw + x] + ((y & 1) ? 2 : 1)) >> 2;
  }
  const int j = x >> 1;
  if (cw <= 2) return p[(int64_t)(vs == 2 ? y >> 1 : y) * pw + j];  // narrow: plain replication
  if (vs == 1) {  // h2v1 fancy
    const uint8_t* r = p + (int64_t)y * pw;
    if (x & 1) return j == cw - 1 ? r[j] : (3 * r[j] + r[j + 1] + 2) >> 2;
    return j == 0 ? r[0] : (3 * r[j] + r[j - 1] + 1) >> 2;
  }
  // h2v2 fancy: column sums of this row and the nearer neighbour row (edge rows repeat), then the horizontal triangle
  const int i = y >> 1, nb = (y & 1) ? min(i + 1, ch - 1) : max(i - 1, 0);
  const uint8_t* r0 = p + (int64_t)i * pw;
  const uint8_t* r1 = p + (int64_t)nb * pw;
  const int cs = 3 * r0[j] + r1[j];
  if (x & 1) return j == cw - 1 ? (cs * 4 + 7) >> 4 : (3 * cs + 3 * r0[j + 1] + r1[j + 1] + 7) >> 4;
  return j == 0 ? (cs * 4 + 8) >> 4 : (3 * cs + 3 * r0[j - 1] + r1[j - 1] + 8) >> 4;
}

__device__ __forceinline__ uint8_t clamp255(int v) { return (uint8_t)min(max(v, 0), 255); }

__global__ __launch_bounds__(256) void od_jpeg_color_k(const od_img_desc* __restrict__ descs, uint8_t* __restrict__ ws) {
  const od_img_desc d = descs[blockIdx.y];
  if (d.kind != OD_IMG_JPEG) return;
  const int W = d.width, H = d.height;
  const int hs = d.ncomp == 1 ? 1 : d.samp_h, vs = d.ncomp == 1 ? 1 : d.samp_v;
  const uint8_t* py = ws + d.plane_ws;
  const int pw0 = d.mcux * hs * 8, pwc = d.mcux * 8;
  const uint8_t* pcb = py + plane_bytes(d, 0);
  const uint8_t* pcr = pcb + plane_bytes(d, 1);
  const int cw = (W + hs - 1) / hs, chh = (H + vs - 1) / vs;
  uint8_t* rgb = ws + d.rgb_ws;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < W * H; i += gridDim.x * 256) {
    const int y = i / W, x = i - y * W;
    const int Y = py[(int64_t)y * pw0 + x];
    uint8_t* o = rgb + (int64_t)i * 3;
    if (d.ncomp == 1) {
      o[0] = o[1] = o[2] = (uint8_t)Y;
      continue;
    }
    const int cb = chroma(pcb, pwc, cw, chh, hs, vs, x, y) - 128;
    const int cr = chroma(pcr, pwc, cw, chh, hs, vs, x, y) - 128;
    o[0] = clamp255(Y + ((91881 * cr + 32768) >> 16));
    o[1] = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    o[2] = clamp255(Y + ((116130 * cb + 32768) >> 16));
  }
}

__device__ __forceinline__ const uint8_t* img_src(const uint8_t* blob, const uint8_t* ws, const od_img_desc& d) {
  return d.kind == OD_IMG_JPEG ? ws + d.rgb_ws : blob + d.src_off;
}

// Image.resize runs the vertical pass first for an image more than 100 times as tall as wide that shrinks vertically
// (the intermediate image is then the small one); the rounding to 8 bits between the passes makes the order visible
__host__ __device__ __forceinline__ bool vertical_first(const od_img_desc& d) {
  return d.height > (int64_t)100 * d.width && d.out_h < d.height;
}

// first pass into tmp.  Horizontal: source [height, width] -> tmp [height, out_w], skipped when out_w == width.
// vertical_first: source -> tmp [out_h, width]
__global__ __launch_bounds__(256) void od_img_hpass_k(const uint8_t* __restrict__ blob, const od_img_desc* __restrict__ descs,
                                                      uint8_t* __restrict__ ws, int kind) {
  const od_img_desc d = descs[blockIdx.y];
  if (d.kind != kind) return;
  const uint8_t* src = img_src(blob, ws, d);
  uint8_t* tmp = ws + d.tmp_ws;
  if (vertical_first(d)) {
    const int* tb = (const int*)(blob + d.vcoef_off);
    const int stride = 2 + d.vk;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < d.out_h * d.width; i += gridDim.x * 256) {
      const int y = i / d.width, x = i - y * d.width;
      const int* t = tb + y * stride;
      resample_px(src + ((int64_t)t[0] * d.width + x) * 3, 3LL * d.width, t, tmp + (int64_t)i * 3);
    }
    return;
  }
  if (d.out_w == d.width) return;
  const int* tb = (const int*)(blob + d.hcoef_off);
  const int ow = d.out_w, stride = 2 + d.hk;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < ow * d.height; i += gridDim.x * 256) {
    const int y = i / ow, xx = i - y * ow;
    const int* t = tb + xx * stride;
    const int x0 = t[0], nt = t[1];
    const uint8_t* s = src + ((int64_t)y * d.width + x0) * 3;
    int64_t a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
    for (int k = 0; k < nt; ++k) {
      const int64_t w = t[2 + k];
      a0 += s[3 * k] * w;
      a1 += s[3 * k + 1] * w;
      a2 += s[3 * k + 2] * w;
    }
    uint8_t* o = tmp + (int64_t)i * 3;
    o[0] = clip8(a0);
    o[1] = clip8(a1);
    o[2] = clip8(a2);
  }
}

// second pass into the canvas: rows < out_h, columns < out_w get the image, the rest zeros.  Vertical over tmp (or the
// source when the horizontal pass was skipped); vertical_first: horizontal over tmp [out_h, width]
__global__ __launch_bounds__(256) void od_img_vpass_k(const uint8_t* __restrict__ blob, const od_img_desc* __restrict__ descs,
                                                      const uint8_t* __restrict__ ws, uint8_t* __restrict__ out, int H,
                                                      int W, int kind) {
  const int b = blockIdx.y;
  const od_img_desc d = descs[b];
  if (d.kind != kind) return;
  const uint8_t* src = d.out_w == d.width ? img_src(blob, ws, d) : ws + d.tmp_ws;  // [height, out_w]
  const int* tb = (const int*)(blob + d.vcoef_off);
  const int ow = d.out_w, stride = 2 + d.vk;
  uint8_t* dst = out + (int64_t)b * H * W * 3;
  const bool vfirst = vertical_first(d);
  const int* htb = (const int*)(blob + d.hcoef_off);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < H * W; i += gridDim.x * 256) {
    const int y = i / W, x = i - y * W;
    uint8_t* o = dst + (int64_t)i * 3;
    if (y >= d.out_h || x >= ow) {
      o[0] = o[1] = o[2] = 0;
      continue;
    }
    if (vfirst) {
      const uint8_t* row = ws + d.tmp_ws + (int64_t)y * d.width * 3;
      if (ow == d.width) {
        o[0] = row[3 * x];
        o[1] = row[3 * x + 1];
        o[2] = row[3 * x + 2];
      } else {
        const int* t = htb + x * (2 + d.hk);
        resample_px(row + (int64_t)t[0] * 3, 3, t, o);
      }
      continue;
    }
    if (d.out_h == d.height) {
      const uint8_t* s = src + ((int64_t)y * ow + x) * 3;
      o[0] = s[0];
      o[1] = s[1];
      o[2] = s[2];
      continue;
    }
    const int* t = tb + y * stride;
    const int y0 = t[0], nt = t[1];
    int64_t a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
    for (int k = 0; k < nt; ++k) {
      const int64_t w = t[2 + k];
      const uint8_t* s = src + ((int64_t)(y0 + k) * ow + x) * 3;
      a0 += s[0] * w;
      a1 += s[1] * w;
      a2 += s[2] * w;
    }
    o[0] = clip8(a0);
    o[1] = clip8(a1);
    o[2] = clip8(a2);
  }
}

int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// the intermediate image between the two resize passes: [height, out_w], or [out_h, width] when vertical_first
int64_t tmp_bytes(const od_img_desc& d) {
  return 3 * (vertical_first(d) ? (int64_t)d.out_h * d.width : (int64_t)d.height * d.out_w);
}

int64_t jpeg_blocks(const od_img_desc& d) {
  return (int64_t)d.mcux * d.mcuy * (d.ncomp == 1 ? 1 : d.samp_h * d.samp_v + 2);
}

// host-side checks of one batch: descriptor sanity and every blob / workspace range in bounds
int check_batch(const od_img_desc* h, int B, long long blob_bytes, long long ws_bytes, int H, int W, int kind,
                int* max_blocks, int* max_pix) {
  *max_blocks = 0;
  *max_pix = 0;
  for (int b = 0; b < B; ++b) {
    const od_img_desc& d = h[b];
    if (d.kind != kind) continue;
    auto in_blob = [&](int64_t off, int64_t n) { return off >= 0 && n >= 0 && off % 16 == 0 && off + n <= blob_bytes; };
    auto in_ws = [&](int64_t off, int64_t n) { return off >= 0 && n >= 0 && off % 16 == 0 && off + n <= ws_bytes; };
    OD_REQUIRE(d.width > 0 && d.height > 0 && d.width <= 65535 && d.height <= 65535 && (int64_t)d.width * d.height <= (1 << 28),
               "od_img: image %d: bad size %dx%d", b, d.width, d.height);
    OD_REQUIRE(d.out_w > 0 && d.out_h > 0 && d.out_w <= W && d.out_h <= H, "od_img: image %d: bad output rectangle", b);
    OD_REQUIRE(d.hk >= 0 && d.vk >= 0 && in_blob(d.hcoef_off, 4LL * d.out_w * (2 + d.hk)) &&
                   in_blob(d.vcoef_off, 4LL * d.out_h * (2 + d.vk)),
               "od_img: image %d: resample tables out of bounds", b);
    const int64_t rgb = 3LL * d.width * d.height;
    OD_REQUIRE(in_ws(d.tmp_ws, tmp_bytes(d)), "od_img: image %d: workspace too small", b);
    if (kind == OD_IMG_RGB) {
      OD_REQUIRE(in_blob(d.src_off, rgb), "od_img: image %d: source out of bounds", b);
    } else {
      OD_REQUIRE((d.ncomp == 1 || (d.ncomp == 3 && d.samp_h >= 1 && d.samp_h <= 2 && d.samp_v >= 1 && d.samp_v <= 2)) &&
                     d.mcux > 0 && d.mcuy > 0 && d.n_sub > 0 && d.stream_bytes >= 0 && d.stream_bytes < (1LL << 28),
                 "od_img: image %d: bad JPEG descriptor", b);
      const int64_t nb = jpeg_blocks(d);
      OD_REQUIRE(nb < (1 << 24), "od_img: image %d: too many blocks", b);
      OD_REQUIRE(in_blob(d.stream_off, d.stream_bytes) && in_blob(d.sub_off, 4LL * OD_JPEG_SUB_INTS * d.n_sub) &&
                     in_blob(d.huff_off, 4LL * 6 * OD_JPEG_HUFF_INTS) && in_blob(d.quant_off, 4LL * 3 * 64),
                 "od_img: image %d: JPEG data out of bounds", b);
      int64_t planes = 0;
      for (int c = 0; c < d.ncomp; ++c) {
        const int hs = (c == 0 && d.ncomp == 3) ? d.samp_h : 1, vs = (c == 0 && d.ncomp == 3) ? d.samp_v : 1;
        planes += (int64_t)d.mcux * hs * 8 * d.mcuy * vs * 8;
      }
      OD_REQUIRE(in_ws(d.coef_ws, nb * 128) && in_ws(d.plane_ws, planes) && in_ws(d.rgb_ws, rgb) &&
                     in_ws(d.state_ws, 16 + 40LL * d.n_sub),
                 "od_img: image %d: workspace too small", b);
      *max_blocks = (int)std::max<int64_t>(*max_blocks, nb);
    }
    *max_pix = std::max(*max_pix, std::max(d.width * d.height, d.out_w * d.height));
  }
  return OD_OK;
}

int grid_x(int64_t n) { return (int)std::min<int64_t>(std::max<int64_t>((n + 255) / 256, 1), 512); }

int resize_batch(const od_img_desc* descs, int B, const uint8_t* blob, uint8_t* ws, uint8_t* out, int H, int W,
                 int max_pix, int kind, hipStream_t s) {
  hipLaunchKernelGGL(od_img_hpass_k, dim3(grid_x(max_pix), B), dim3(256), 0, s, blob, descs, ws, kind);
  OD_CHECK_LAUNCH();
  hipLaunchKernelGGL(od_img_vpass_k, dim3(grid_x((int64_t)H * W), B), dim3(256), 0, s, blob, descs, ws, out, H, W, kind);
  OD_CHECK_LAUNCH();
  return OD_OK;
}

}  // namespace

extern "C" int od_img_workspace_plan(od_img_desc* descs_host, int B, long long* workspace_bytes) {
  OD_REQUIRE(descs_host && workspace_bytes && B > 0, "od_img_workspace_plan: bad argument");
  int64_t off = 0;
  for (int b = 0; b < B; ++b) {
    od_img_desc& d = descs_host[b];
    d.coef_ws = d.plane_ws = d.rgb_ws = d.state_ws = 0;
    if (d.kind == OD_IMG_JPEG) {
      d.coef_ws = off;
      off = align256(off + jpeg_blocks(d) * 128);
      d.plane_ws = off;
      for (int c = 0; c < d.ncomp; ++c) {
        const int hs = (c == 0 && d.ncomp == 3) ? d.samp_h : 1, vs = (c == 0 && d.ncomp == 3) ? d.samp_v : 1;
        off += (int64_t)d.mcux * hs * 8 * d.mcuy * vs * 8;
      }
      off = align256(off);
      d.rgb_ws = off;
      off = align256(off + 3LL * d.width * d.height);
      d.state_ws = off;
      off = align256(off + 16 + 40LL * d.n_sub);
    }
    d.tmp_ws = off;
    off = align256(off + tmp_bytes(d));
  }
  *workspace_bytes = off;
  return OD_OK;
}

extern "C" int od_jpeg_decode_resize(od_ctx* ctx, const od_img_desc* descs_host, const od_img_desc* descs, int B,
                                     const uint8_t* blob, long long blob_bytes, void* workspace, long long ws_bytes,
                                     uint8_t* out, int H, int W, void* stream) {
  OD_REQUIRE(ctx && descs_host && descs && blob && workspace && out && B > 0 && B <= 65535 && H > 0 && W > 0,
             "od_jpeg_decode_resize: bad argument");
  int max_blocks, max_pix;
  const int rc = check_batch(descs_host, B, blob_bytes, ws_bytes, H, W, OD_IMG_JPEG, &max_blocks, &max_pix);
  if (rc != OD_OK) return rc;
  if (max_pix == 0) return OD_OK;  // no JPEG in this batch
  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)workspace;
  hipLaunchKernelGGL(od_jpeg_huff_k, dim3(B), dim3(HT), 0, s, blob, descs, ws);
  OD_CHECK_LAUNCH();
  hipLaunchKernelGGL(od_jpeg_idct_k, dim3(grid_x(max_blocks), B), dim3(256), 0, s, blob, descs, ws);
  OD_CHECK_LAUNCH();
  hipLaunchKernelGGL(od_jpeg_color_k, dim3(grid_x(max_pix), B), dim3(256), 0, s, descs, ws);
  OD_CHECK_LAUNCH();
  return resize_batch(descs, B, blob, ws, out, H, W, max_pix, OD_IMG_JPEG, s);
}

extern "C" int od_rgb_resize(od_ctx* ctx, const od_img_desc* descs_host, const od_img_desc* descs, int B,
                             const uint8_t* blob, long long blob_bytes, void* workspace, long long ws_bytes, uint8_t* out,
                             int H, int W, void* stream) {
  OD_REQUIRE(ctx && descs_host && descs && blob && workspace && out && B > 0 && B <= 65535 && H > 0 && W > 0,
             "od_rgb_resize: bad argument");
  int max_blocks, max_pix;
  const int rc = check_batch(descs_host, B, blob_bytes, ws_bytes, H, W, OD_IMG_RGB, &max_blocks, &max_pix);
  if (rc != OD_OK) return rc;
  if (max_pix == 0) return OD_OK;
  return resize_batch(descs, B, blob, (uint8_t*)workspace, out, H, W, max_pix, OD_IMG_RGB, (hipStream_t)stream);
}
