// The Inferencer's visualisation on the GPU: predictions drawn on the uploaded original images, in place.
//
// draw_detections_kernel  replaces DetLocalVisualizer.add_datasample as the reference's Inferencer.visualize drives it
//                     (codetr/inferencer.py:163-235, called at :458-470; matplotlib + cv2 on the host) with this
//                     library's own rendering, stated in integer pixel arithmetic in include/codetr_hip.h: per drawn
//                     detection a box outline blended in its class colour, then -- after every outline of the image --
//                     "<name>: <percent>" in a 5x7 bitmap font on a darkened patch at the box's corner.
// Gather form: one 256-thread workgroup owns a 64x16-pixel tile of one image (a wave = 64 consecutive pixels of a row,
// 192 contiguous bytes; four rows per thread) and applies, in ascending detection order, every outline and then every
// label that reaches its tile.  Each pixel has one owner, so the order is the contract's and nothing races.
//   Phase 1  the workgroup walks the image's detection rows 256 at a time and appends the index of every drawn row whose
//            edge band meets the tile to one LDS list, of every one whose text grid meets it to a second one (uint16
//            entries, 4096 each: 16 KB).  Order is kept by a 64-bit ballot, the count of set lower lanes and a per-wave
//            base exchanged through LDS (two alternating slots: one barrier per 256 rows).
//   Phase 2  a tile with two empty lists returns without touching the image.  Otherwise each thread loads its four
//            pixels, runs the edge list and then the label list -- the entry is made wave-uniform, so a detection's box,
//            score and label come through the scalar cache -- and stores the pixels that changed, byte by byte (image
//            offsets and row pitches are not dword-aligned in general).
// A separate translation unit from prepost.hip on purpose: the code of the post-processing kernels there is pinned.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "codetr_hip.h"
#include "box_prims.h"

// The 5x7 font, authored for this library: ASCII 32..126, 7 bytes per glyph, top row first, bit 4 = the leftmost pixel.
// One initialiser for the kernel's __constant__ copy and for the host copy that codetr_draw_font hands out.
#define CODETR_DRAW_FONT_ROWS \
  0x00,0x00,0x00,0x00,0x00,0x00,0x00,  0x04,0x04,0x04,0x04,0x04,0x00,0x04,  0x0a,0x0a,0x0a,0x00,0x00,0x00,0x00,  0x0a,0x0a,0x1f,0x0a,0x1f,0x0a,0x0a, /* sp ! " # */ \
  0x04,0x0f,0x14,0x0e,0x05,0x1e,0x04,  0x18,0x19,0x02,0x04,0x08,0x13,0x03,  0x0c,0x12,0x14,0x08,0x15,0x12,0x0d,  0x04,0x04,0x08,0x00,0x00,0x00,0x00, /* $ % & ' */ \
  0x02,0x04,0x08,0x08,0x08,0x04,0x02,  0x08,0x04,0x02,0x02,0x02,0x04,0x08,  0x00,0x04,0x15,0x0e,0x15,0x04,0x00,  0x00,0x04,0x04,0x1f,0x04,0x04,0x00, /* ( ) * + */ \
  0x00,0x00,0x00,0x00,0x0c,0x04,0x08,  0x00,0x00,0x00,0x1f,0x00,0x00,0x00,  0x00,0x00,0x00,0x00,0x00,0x0c,0x0c,  0x00,0x01,0x02,0x04,0x08,0x10,0x00, /* , - . / */ \
  0x0e,0x11,0x13,0x15,0x19,0x11,0x0e,  0x04,0x0c,0x04,0x04,0x04,0x04,0x0e,  0x0e,0x11,0x01,0x02,0x04,0x08,0x1f,  0x1f,0x02,0x04,0x02,0x01,0x11,0x0e, /* 0 1 2 3 */ \
  0x02,0x06,0x0a,0x12,0x1f,0x02,0x02,  0x1f,0x10,0x1e,0x01,0x01,0x11,0x0e,  0x06,0x08,0x10,0x1e,0x11,0x11,0x0e,  0x1f,0x01,0x02,0x04,0x08,0x08,0x08, /* 4 5 6 7 */ \
  0x0e,0x11,0x11,0x0e,0x11,0x11,0x0e,  0x0e,0x11,0x11,0x0f,0x01,0x02,0x0c,  0x00,0x0c,0x0c,0x00,0x0c,0x0c,0x00,  0x00,0x0c,0x0c,0x00,0x0c,0x04,0x08, /* 8 9 : ; */ \
  0x02,0x04,0x08,0x10,0x08,0x04,0x02,  0x00,0x00,0x1f,0x00,0x1f,0x00,0x00,  0x08,0x04,0x02,0x01,0x02,0x04,0x08,  0x0e,0x11,0x01,0x02,0x04,0x00,0x04, /* < = > ? */ \
  0x0e,0x11,0x01,0x0d,0x15,0x15,0x0e,  0x0e,0x11,0x11,0x11,0x1f,0x11,0x11,  0x1e,0x11,0x11,0x1e,0x11,0x11,0x1e,  0x0e,0x11,0x10,0x10,0x10,0x11,0x0e, /* @ A B C */ \
  0x1c,0x12,0x11,0x11,0x11,0x12,0x1c,  0x1f,0x10,0x10,0x1e,0x10,0x10,0x1f,  0x1f,0x10,0x10,0x1e,0x10,0x10,0x10,  0x0e,0x11,0x10,0x17,0x11,0x11,0x0f, /* D E F G */ \
  0x11,0x11,0x11,0x1f,0x11,0x11,0x11,  0x0e,0x04,0x04,0x04,0x04,0x04,0x0e,  0x07,0x02,0x02,0x02,0x02,0x12,0x0c,  0x11,0x12,0x14,0x18,0x14,0x12,0x11, /* H I J K */ \
  0x10,0x10,0x10,0x10,0x10,0x10,0x1f,  0x11,0x1b,0x15,0x15,0x11,0x11,0x11,  0x11,0x11,0x19,0x15,0x13,0x11,0x11,  0x0e,0x11,0x11,0x11,0x11,0x11,0x0e, /* L M N O */ \
  0x1e,0x11,0x11,0x1e,0x10,0x10,0x10,  0x0e,0x11,0x11,0x11,0x15,0x12,0x0d,  0x1e,0x11,0x11,0x1e,0x14,0x12,0x11,  0x0f,0x10,0x10,0x0e,0x01,0x01,0x1e, /* P Q R S */ \
  0x1f,0x04,0x04,0x04,0x04,0x04,0x04,  0x11,0x11,0x11,0x11,0x11,0x11,0x0e,  0x11,0x11,0x11,0x11,0x11,0x0a,0x04,  0x11,0x11,0x11,0x15,0x15,0x15,0x0a, /* T U V W */ \
  0x11,0x11,0x0a,0x04,0x0a,0x11,0x11,  0x11,0x11,0x11,0x0a,0x04,0x04,0x04,  0x1f,0x01,0x02,0x04,0x08,0x10,0x1f,  0x0e,0x08,0x08,0x08,0x08,0x08,0x0e, /* X Y Z [ */ \
  0x00,0x10,0x08,0x04,0x02,0x01,0x00,  0x0e,0x02,0x02,0x02,0x02,0x02,0x0e,  0x04,0x0a,0x11,0x00,0x00,0x00,0x00,  0x00,0x00,0x00,0x00,0x00,0x00,0x1f, /* backslash ] ^ _ */ \
  0x08,0x04,0x02,0x00,0x00,0x00,0x00,  0x00,0x00,0x0e,0x01,0x0f,0x11,0x0f,  0x10,0x10,0x16,0x19,0x11,0x11,0x1e,  0x00,0x00,0x0e,0x10,0x10,0x11,0x0e, /* ` a b c */ \
  0x01,0x01,0x0d,0x13,0x11,0x11,0x0f,  0x00,0x00,0x0e,0x11,0x1f,0x10,0x0e,  0x06,0x09,0x08,0x1c,0x08,0x08,0x08,  0x00,0x0f,0x11,0x11,0x0f,0x01,0x0e, /* d e f g */ \
  0x10,0x10,0x16,0x19,0x11,0x11,0x11,  0x04,0x00,0x0c,0x04,0x04,0x04,0x0e,  0x02,0x00,0x06,0x02,0x02,0x12,0x0c,  0x10,0x10,0x12,0x14,0x18,0x14,0x12, /* h i j k */ \
  0x0c,0x04,0x04,0x04,0x04,0x04,0x0e,  0x00,0x00,0x1a,0x15,0x15,0x11,0x11,  0x00,0x00,0x16,0x19,0x11,0x11,0x11,  0x00,0x00,0x0e,0x11,0x11,0x11,0x0e, /* l m n o */ \
  0x00,0x1e,0x11,0x11,0x1e,0x10,0x10,  0x00,0x0f,0x11,0x11,0x0f,0x01,0x01,  0x00,0x00,0x16,0x19,0x10,0x10,0x10,  0x00,0x00,0x0f,0x10,0x0e,0x01,0x1e, /* p q r s */ \
  0x08,0x08,0x1c,0x08,0x08,0x09,0x06,  0x00,0x00,0x11,0x11,0x11,0x13,0x0d,  0x00,0x00,0x11,0x11,0x11,0x0a,0x04,  0x00,0x00,0x11,0x11,0x15,0x15,0x0a, /* t u v w */ \
  0x00,0x00,0x11,0x0a,0x04,0x0a,0x11,  0x00,0x11,0x11,0x11,0x0f,0x01,0x0e,  0x00,0x00,0x1f,0x02,0x04,0x08,0x1f,  0x02,0x04,0x04,0x08,0x04,0x04,0x02, /* x y z { */ \
  0x04,0x04,0x04,0x04,0x04,0x04,0x04,  0x08,0x04,0x04,0x02,0x04,0x04,0x08,  0x00,0x00,0x08,0x15,0x02,0x00,0x00, /* | } ~ */ \

namespace {

constexpr int kTileW = 64, kTileH = 16, kRowsPerThread = 4;
constexpr int kDrawMaxQ = CODETR_DRAW_MAX_Q;
constexpr int kNameRow = 24;  // bytes per row of the names table: the length, then up to 23 characters
static_assert(kDrawMaxQ <= 65536, "the LDS lists hold uint16 indices");

__constant__ unsigned char d_font[CODETR_DRAW_FONT_BYTES] = {CODETR_DRAW_FONT_ROWS};
const unsigned char h_font[CODETR_DRAW_FONT_BYTES] = {CODETR_DRAW_FONT_ROWS};

struct DrawImage {
  int64_t offset;
  int H, W;
};
struct DrawTable {  // a kernel argument, like prepost.hip's BatchTable (512 B)
  DrawImage img[CODETR_PREPROCESS_BATCH_MAX];
};
struct DrawStyle {
  int lw, A, font_scale, draw_labels;
  float score_thr;
  int text[3];
};

// one drawn detection in pixel units
struct Det {
  int x1, y1, x2, y2;
};

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// clamp in fp32 to [-16384, 16383], then (int)floorf(x + 0.5f): one fp32 rounding in the sum
__device__ __forceinline__ int pixel_coord(float v) {
#pragma clang fp contract(off)
  v = fminf(fmaxf(v, -16384.f), 16383.f);
  return (int)floorf(v + 0.5f);
}

template <class T>
__device__ __forceinline__ Det pixel_box(const T* __restrict__ box) {
  return Det{pixel_coord(to_f32(box[0])), pixel_coord(to_f32(box[1])), pixel_coord(to_f32(box[2])),
             pixel_coord(to_f32(box[3]))};
}

// tenths of a percent: score * 1000 + 0.5 with a rounding after each operation, clamped in fp32, truncated
__device__ __forceinline__ int score_tenths(float s) {
#pragma clang fp contract(off)
  const float m = s * 1000.0f;
  const float v = m + 0.5f;
  return !(v > 0.f) ? 0 : v >= 1000.f ? 1000 : (int)v;
}
__device__ __forceinline__ int int_digits(int tenths) { return tenths >= 1000 ? 3 : tenths >= 100 ? 2 : 1; }

__device__ __forceinline__ int name_length(const unsigned char* __restrict__ names, int label) {
  const int len = names[(size_t)label * kNameRow];
  return len > kNameRow - 1 ? kNameRow - 1 : len;
}

__device__ __forceinline__ int text_scale(Det d, int font_scale) {
  return font_scale * (1 + ((d.x2 - d.x1) * (d.y2 - d.y1) >= 15400 ? 1 : 0));
}

__device__ __forceinline__ int blend(int p, int c, int A) { return (p * (256 - A) + c * A + 128) >> 8; }

// how many set bits of a ballot sit below this lane
__device__ __forceinline__ int lower_lanes(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// grid (ceil(Wmax / 64), ceil(Hmax / 16), N)
template <class T>
__global__ __launch_bounds__(256) void draw_detections_kernel(unsigned char* __restrict__ buf, DrawTable tab,
                                                              const T* __restrict__ boxes, const T* __restrict__ scores,
                                                              const int64_t* __restrict__ labels,
                                                              const int* __restrict__ count, int Q,
                                                              const unsigned char* __restrict__ palette,
                                                              const unsigned char* __restrict__ names, int C,
                                                              DrawStyle st) {
  __shared__ unsigned short s_edge[kDrawMaxQ], s_text[kDrawMaxQ];
  __shared__ int s_cnt[2][2][4];
  const int n = blockIdx.z;
  const DrawImage im = tab.img[n];
  const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
  if (tx0 >= im.W || ty0 >= im.H) return;  // a tile beyond its image (uniform)
  const int tx1 = min(tx0 + kTileW, im.W) - 1, ty1 = min(ty0 + kTileH, im.H) - 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a = st.lw / 2, b = (st.lw - 1) / 2;
  const T* ibox = boxes + (size_t)n * Q * 4;
  const T* iscore = scores + (size_t)n * Q;
  const int64_t* ilabel = labels + (size_t)n * Q;
  const int cnt = min(max(count[n], 0), Q);

  // ---- phase 1: which detections reach this tile, in ascending order
  int ne = 0, nt = 0;  // (uniform)
  for (int base = 0, it = 0; base < cnt; base += 256, it ^= 1) {
    const int j = base + tid;
    bool edge = false, text = false;
    if (j < cnt) {
      const float s = to_f32(iscore[j]);
      const int64_t label = ilabel[j];
      const float x1 = to_f32(ibox[4 * j]), y1 = to_f32(ibox[4 * j + 1]);
      const float x2 = to_f32(ibox[4 * j + 2]), y2 = to_f32(ibox[4 * j + 3]);
      if (s > st.score_thr && label >= 0 && label < C && finite_f(x1) && finite_f(y1) && finite_f(x2) && finite_f(y2)) {
        const Det d{pixel_coord(x1), pixel_coord(y1), pixel_coord(x2), pixel_coord(y2)};
        if (d.x2 >= d.x1 && d.y2 >= d.y1) {
          // the band's outer rectangle meets the tile and the tile is not wholly inside the inner one
          const bool outer = d.x1 - a <= tx1 && d.x2 + a >= tx0 && d.y1 - a <= ty1 && d.y2 + a >= ty0;
          const bool inner = tx0 >= d.x1 + b + 1 && tx1 <= d.x2 - b - 1 && ty0 >= d.y1 + b + 1 && ty1 <= d.y2 - b - 1;
          edge = outer && !inner;
          if (st.draw_labels) {
            const int len = name_length(names, (int)label) + 2 + int_digits(score_tenths(s)) + 2;
            const int sc = text_scale(d, st.font_scale);
            const int ox = d.x1 + st.lw, oy = d.y1 + st.lw;
            text = ox <= tx1 && ox + (6 * len + 1) * sc - 1 >= tx0 && oy <= ty1 && oy + 9 * sc - 1 >= ty0;
          }
        }
      }
    }
    const unsigned long long me = __ballot(edge), mt = __ballot(text);
    if (lane == 0) {
      s_cnt[it][0][wave] = __popcll(me);
      s_cnt[it][1][wave] = __popcll(mt);
    }
    __syncthreads();
    int be = ne, bt = nt;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int ce = s_cnt[it][0][w], ct = s_cnt[it][1][w];
      if (w < wave) {
        be += ce;
        bt += ct;
      }
      ne += ce;
      nt += ct;
    }
    if (edge) s_edge[be + lower_lanes(me)] = (unsigned short)j;
    if (text) s_text[bt + lower_lanes(mt)] = (unsigned short)j;
  }
  __syncthreads();
  if (ne == 0 && nt == 0) return;

  // ---- phase 2: this thread's pixels: column x, rows y[0..3]
  const int x = tx0 + lane;
  const bool col_ok = x <= tx1;
  unsigned char* img = buf + im.offset;
  int p[kRowsPerThread][3];
  bool touched[kRowsPerThread];
#pragma unroll
  for (int r = 0; r < kRowsPerThread; ++r) {
    const int y = ty0 + wave * kRowsPerThread + r;
    touched[r] = false;
    p[r][0] = p[r][1] = p[r][2] = 0;
    if (col_ok && y <= ty1) {
      const unsigned char* q = img + ((size_t)y * im.W + x) * 3;
      p[r][0] = q[0];
      p[r][1] = q[1];
      p[r][2] = q[2];
    }
  }

  for (int i = 0; i < ne; ++i) {
    const int j = __builtin_amdgcn_readfirstlane((int)s_edge[i]);
    const Det d = pixel_box(ibox + 4 * j);
    const int label = (int)ilabel[j];
    const int c0 = palette[3 * label], c1 = palette[3 * label + 1], c2 = palette[3 * label + 2];
    if (x < d.x1 - a || x > d.x2 + a) continue;
    const bool x_inner = x >= d.x1 + b + 1 && x <= d.x2 - b - 1;
#pragma unroll
    for (int r = 0; r < kRowsPerThread; ++r) {
      const int y = ty0 + wave * kRowsPerThread + r;
      const bool on = y >= d.y1 - a && y <= d.y2 + a && !(x_inner && y >= d.y1 + b + 1 && y <= d.y2 - b - 1);
      if (on) {
        p[r][0] = blend(p[r][0], c0, st.A);
        p[r][1] = blend(p[r][1], c1, st.A);
        p[r][2] = blend(p[r][2], c2, st.A);
        touched[r] = true;
      }
    }
  }

  for (int i = 0; i < nt; ++i) {
    const int j = __builtin_amdgcn_readfirstlane((int)s_text[i]);
    const Det d = pixel_box(ibox + 4 * j);
    const int label = (int)ilabel[j];
    const int tenths = score_tenths(to_f32(iscore[j]));
    const unsigned char* name = names + (size_t)label * kNameRow;
    const int nlen = name_length(names, label), nd = int_digits(tenths);
    const int len = nlen + 2 + nd + 2;
    const int sc = text_scale(d, st.font_scale);
    const int gx = x - (d.x1 + st.lw);
    if (gx < 0 || gx >= (6 * len + 1) * sc) continue;
    const int fx = gx / sc;
    // the character of this column and the bit of its glyph row that the column shows (none between characters)
    const int k = fx >= 1 ? (fx - 1) / 6 : 0, col = fx >= 1 ? (fx - 1) - 6 * k : 5;
    int ch;
    if (k < nlen) {
      ch = name[1 + k];
    } else {
      const int t = k - nlen;  // ": " then the integer part, ".", the tenth
      const int whole = tenths / 10;
      if (t == 0) ch = ':';
      else if (t == 1) ch = ' ';
      else if (t == 2 + nd) ch = '.';
      else if (t == 3 + nd) ch = '0' + tenths % 10;
      else {
        const int pos = nd - 1 - (t - 2);  // 0 = units
        ch = '0' + (pos == 0 ? whole % 10 : pos == 1 ? (whole / 10) % 10 : whole / 100);
      }
    }
    if (ch < 32 || ch > 126) ch = '?';
    const unsigned char* glyph = d_font + (ch - 32) * 7;
#pragma unroll
    for (int r = 0; r < kRowsPerThread; ++r) {
      const int y = ty0 + wave * kRowsPerThread + r;
      const int gy = y - (d.y1 + st.lw);
      if (gy < 0 || gy >= 9 * sc) continue;
      const int fy = gy / sc;
      const bool ink = col < 5 && fy >= 1 && fy <= 7 && ((glyph[fy >= 1 && fy <= 7 ? fy - 1 : 0] >> (4 - col)) & 1);
      if (ink) {
        p[r][0] = st.text[0];
        p[r][1] = st.text[1];
        p[r][2] = st.text[2];
      } else {
        p[r][0] = blend(p[r][0], 0, st.A);
        p[r][1] = blend(p[r][1], 0, st.A);
        p[r][2] = blend(p[r][2], 0, st.A);
      }
      touched[r] = true;
    }
  }

#pragma unroll
  for (int r = 0; r < kRowsPerThread; ++r) {
    const int y = ty0 + wave * kRowsPerThread + r;
    if (touched[r] && col_ok && y <= ty1) {
      unsigned char* q = img + ((size_t)y * im.W + x) * 3;
      q[0] = (unsigned char)p[r][0];
      q[1] = (unsigned char)p[r][1];
      q[2] = (unsigned char)p[r][2];
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

template <class T>
int launch_draw(void* stream, void* buf, int64_t buf_bytes, int64_t N, const int64_t* images, const void* boxes,
                const void* scores, const int64_t* labels, const int* count, int64_t Q, const unsigned char* palette,
                const unsigned char* names, int64_t C, int line_width, float alpha, float score_thr, uint32_t text_rgb,
                int font_scale, int draw_labels) {
  if (!buf || !images || !boxes || !scores || !labels || !count || !palette || !names || buf_bytes <= 0 || N <= 0 ||
      Q <= 0 || C <= 0)
    return CODETR_E_BADARG;
  if (line_width < 1 || line_width > 15 || !(alpha >= 0.f && alpha <= 1.f) || score_thr != score_thr ||
      text_rgb > 0xffffffu || font_scale < 1 || font_scale > 4 || (draw_labels != 0 && draw_labels != 1))
    return CODETR_E_BADARG;
  if (N > CODETR_PREPROCESS_BATCH_MAX || Q > kDrawMaxQ || C > 65536) return CODETR_E_TOO_LARGE;
  DrawTable tab = {};
  int64_t Hmax = 0, Wmax = 0;
  for (int64_t n = 0; n < N; ++n) {
    const int64_t off = images[3 * n], H = images[3 * n + 1], W = images[3 * n + 2];
    if (off < 0 || H <= 0 || W <= 0) return CODETR_E_BADARG;
    if (H > CODETR_DRAW_MAX_SIDE || W > CODETR_DRAW_MAX_SIDE) return CODETR_E_TOO_LARGE;
    if (off > buf_bytes || H * W * 3 > buf_bytes - off) return CODETR_E_BADARG;  // the image must lie in the buffer
    for (int64_t m = 0; m < n; ++m) {  // in place: two images may not share a byte
      const int64_t o2 = tab.img[m].offset, e2 = o2 + (int64_t)tab.img[m].H * tab.img[m].W * 3;
      if (off < e2 && o2 < off + H * W * 3) return CODETR_E_BADARG;
    }
    tab.img[n] = DrawImage{off, (int)H, (int)W};
    Hmax = H > Hmax ? H : Hmax;
    Wmax = W > Wmax ? W : Wmax;
  }
  DrawStyle st;
  st.lw = line_width;
  st.A = (int)(alpha * 256.0f + 0.5f);
  st.font_scale = font_scale;
  st.draw_labels = draw_labels;
  st.score_thr = score_thr;
  st.text[0] = (int)((text_rgb >> 16) & 255u);
  st.text[1] = (int)((text_rgb >> 8) & 255u);
  st.text[2] = (int)(text_rgb & 255u);
  const dim3 grid((unsigned)((Wmax + kTileW - 1) / kTileW), (unsigned)((Hmax + kTileH - 1) / kTileH), (unsigned)N);
  hipLaunchKernelGGL((draw_detections_kernel<T>), grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<unsigned char*>(buf), tab, static_cast<const T*>(boxes), static_cast<const T*>(scores),
                     labels, count, (int)Q, palette, names, (int)C, st);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

}  // namespace

extern "C" {

int codetr_draw_font(unsigned char* out_host) {
  if (!out_host) return CODETR_E_BADARG;
  memcpy(out_host, h_font, sizeof(h_font));
  return 0;
}

#define CODETR_DRAW_ENTRY(SUFFIX, TYPE)                                                                                  \
  int codetr_draw_detections_##SUFFIX(void* stream, void* buf_dev, int64_t buf_bytes, int64_t N,                         \
                                      const int64_t* images_host, const void* boxes_dev, const void* scores_dev,        \
                                      const int64_t* labels_dev, const int* count_dev, int64_t Q,                        \
                                      const unsigned char* palette_dev, const unsigned char* names_dev, int64_t C,       \
                                      int line_width, float alpha, float score_thr, uint32_t text_rgb, int font_scale,   \
                                      int draw_labels) {                                                                 \
    return launch_draw<TYPE>(stream, buf_dev, buf_bytes, N, images_host, boxes_dev, scores_dev, labels_dev, count_dev,  \
                             Q, palette_dev, names_dev, C, line_width, alpha, score_thr, text_rgb, font_scale,           \
                             draw_labels);                                                                               \
  }
CODETR_DRAW_ENTRY(f16, _Float16)
CODETR_DRAW_ENTRY(bf16, Bf16)
CODETR_DRAW_ENTRY(f32, float)
#undef CODETR_DRAW_ENTRY

}  // extern "C"
