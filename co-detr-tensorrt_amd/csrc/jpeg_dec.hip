// Baseline JPEG decoder (C ABI and the whole rule: include/codetr_jpeg_dec.h; the symbol step, IDCT, upsampling and colour:
// jpeg_dec_core.h; the header parser: jpeg_dec_parse.h).
//
// Huffman decoding is sequential as written; here it is the self-synchronising chunked decode.  The scan is cut into
// chunks of 64 raw bytes, one lane per chunk; a lane owns the symbols that start in its chunk and its entry state is
// (bit position, block of the MCU, zigzag index).  Every lane starts from the guess "first bit of the chunk, block 0,
// index 0"; a lane's exit state is the next lane's entry state, and a lane whose entry state changed decodes again.
// After round r the first r chunks are final, so the fixed point is the sequential decode and takes at most one round
// per chunk whatever the speculation met (codes that match nothing included: only the final pass reports).
//   1 jpegdec_sync_runs      one workgroup per run of 256 chunks: the fixed point inside the run, exchanged through LDS
//   2 jpegdec_link_runs      one workgroup per image: walks the runs in order, repairs those whose guessed entry was
//                            wrong (usually their first chunks only), then scans block counts and DC sums over the chunks
//   3 jpegdec_coefficients   every lane decodes once more from its final state: coefficients (DC absolute), status
//   4 jpegdec_idct           dequantisation + IDCT of every block into its component's plane
//   5 jpegdec_pixels         upsampling + colour, one thread per pixel, packed RGB
// Workgroups never talk to each other inside a launch; all exchange is through the launch boundaries.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codetr_hip.h"
#include "codetr_jpeg_dec.h"
#include "jpeg_dec_core.h"
#include "jpeg_dec_parse.h"

namespace {

using namespace jpegdec;

constexpr int kThreads = kRun;   // a lane per chunk of a run
constexpr int kRecInts = 16;     // a chunk's record in the workspace
// record: 0 entry pos, 1 entry mk, 2 exit pos, 3 exit mk, 4 blocks, 5 reset, 6..8 dc sums, 9 first block, 10..12 predictors
constexpr int kIdctBlocks = 32;  // blocks per workgroup of the IDCT (8 lanes each)

struct DecImage {
  int64_t scan_off, dst_off, rec_off, coef_off, plane_off;   // byte offsets: scans_dev, dst_dev, workspace x 3
  int H, W, scan_len, dri, nchunks, mcus_x, mcus_y, nblocks;
  unsigned char ncomp, bpm, hmax, vmax, tq[3], td[3], ta[3], pad[3];
};

struct DecTable {
  DecImage img[CODETR_PREPROCESS_BATCH_MAX];
};

__device__ const unsigned char kNaturalDev[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// plane of component c: blocks across, blocks down, byte offset behind the image's plane_off
__host__ __device__ inline void plane_of(const DecImage& im, int c, int* bw, int* bh, int64_t* off) {
  const int64_t y_bytes = (int64_t)im.mcus_x * im.hmax * im.mcus_y * im.vmax * 64, c_bytes = (int64_t)im.mcus_x * im.mcus_y * 64;
  if (c == 0) {
    *bw = im.mcus_x * im.hmax;
    *bh = im.mcus_y * im.vmax;
    *off = 0;
  } else {
    *bw = im.mcus_x;
    *bh = im.mcus_y;
    *off = y_bytes + (c - 1) * c_bytes;
  }
}

__device__ inline void load_tables(const DecImage& im, const unsigned char* tables, Huff* h, unsigned char* natural, Scan* s,
                                   const unsigned char* scans) {
  const int t = threadIdx.x;
  if (t < 8) huff_build(tables + kQuantBytes + t * kHuffBytes, t, h);
  if (t >= 64 && t < 128) natural[t - 64] = kNaturalDev[t - 64];
  s->data = scans + im.scan_off;
  s->len = im.scan_len;
  s->dri = im.dri;
  s->bpm = im.bpm;
  s->nblocks = im.nblocks;
  for (int i = 0; i < 6; ++i) s->comp[i] = (unsigned char)(im.ncomp == 1 ? 0 : (i < im.bpm - 2 ? 0 : i - (im.bpm - 2) + 1));
  for (int c = 0; c < 3; ++c) {
    s->td[c] = im.td[c];
    s->ta[c] = im.ta[c];
  }
  __syncthreads();
}

// The fixed point over the 256 chunks of one run.  `entry` / `lane`: this lane's entry state and what it decoded from it
// (from a guess, or from the records of an earlier launch); dirty: this lane has to decode.  Records go to rec.
__device__ inline void run_fixed_point(const Scan& s, const Huff& h, const unsigned char* natural, int chunk, int nchunks,
                                       int* rec, int epos, int emk, Lane lane, bool dirty, int* s_pos, int* s_mk) {
  const int t = threadIdx.x;
  const bool valid = chunk < nchunks;
  const int chunk_end = chunk == nchunks - 1 ? 0x7FFFFFFF : (chunk + 1) * kChunk;
  for (int round = 0; round <= kRun; ++round) {   // (round r fixes lane r at the latest)
    if (dirty && valid) {
      decode_chunk<false>(s, h, natural, epos, emk, chunk * kChunk, chunk_end, 0, nullptr, nullptr, &lane);
      int* r = rec + (int64_t)chunk * kRecInts;
      r[0] = epos;
      r[1] = emk;
      r[2] = lane.pos;
      r[3] = lane.mk;
      r[4] = lane.nblk;
      r[5] = lane.reset;
      r[6] = lane.dc[0];
      r[7] = lane.dc[1];
      r[8] = lane.dc[2];
    }
    s_pos[t] = lane.pos;
    s_mk[t] = lane.mk;
    __syncthreads();
    dirty = false;
    if (t > 0 && valid) {
      const int np = s_pos[t - 1], nm = s_mk[t - 1];
      dirty = np != epos || nm != emk;
      epos = np;
      emk = nm;
    }
    if (!__syncthreads_or(dirty ? 1 : 0)) break;
  }
}

__global__ __launch_bounds__(kThreads) void jpegdec_sync_runs(DecTable tab, const unsigned char* scans, const unsigned char* tables,
                                                               unsigned char* ws) {
  __shared__ Huff h;
  __shared__ unsigned char natural[64];
  __shared__ int s_pos[kThreads], s_mk[kThreads];
  const DecImage& im = tab.img[blockIdx.y];
  const int run = blockIdx.x;
  if (run * kRun >= im.nchunks) return;   // (uniform over the workgroup)
  Scan s;
  load_tables(im, tables + (int64_t)blockIdx.y * CODETR_JPEGDEC_TABLE_BYTES, &h, natural, &s, scans);
  const int chunk = run * kRun + threadIdx.x;
  Lane lane = {};
  run_fixed_point(s, h, natural, chunk, im.nchunks, reinterpret_cast<int*>(ws + im.rec_off), chunk * kChunk * 8, 0, lane, true,
                  s_pos, s_mk);
}

__global__ __launch_bounds__(kThreads) void jpegdec_link_runs(DecTable tab, const unsigned char* scans, const unsigned char* tables,
                                                               unsigned char* ws) {
  __shared__ Huff h;
  __shared__ unsigned char natural[64];
  __shared__ int s_pos[kThreads], s_mk[kThreads];
  __shared__ int s_carry[2];
  __shared__ int s_sum[kThreads][5];   // per thread: blocks, reset, dc sums of its chunks; then the exclusive scan
  const DecImage& im = tab.img[blockIdx.x];
  Scan s;
  load_tables(im, tables + (int64_t)blockIdx.x * CODETR_JPEGDEC_TABLE_BYTES, &h, natural, &s, scans);
  int* rec = reinterpret_cast<int*>(ws + im.rec_off);
  const int t = threadIdx.x, nruns = (im.nchunks + kRun - 1) / kRun;
  for (int run = 1; run < nruns; ++run) {
    const int chunk = run * kRun + t;
    if (t == 0) {   // the exit of the chunk in front of the run is final by now
      s_carry[0] = rec[(int64_t)(chunk - 1) * kRecInts + 2];
      s_carry[1] = rec[(int64_t)(chunk - 1) * kRecInts + 3];
    }
    __syncthreads();
    int epos = 0, emk = 0;
    Lane lane = {};
    if (chunk < im.nchunks) {
      const int* r = rec + (int64_t)chunk * kRecInts;
      epos = r[0];
      emk = r[1];
      lane.pos = r[2];
      lane.mk = r[3];
    }
    bool dirty = false;
    if (t == 0) {
      dirty = s_carry[0] != epos || s_carry[1] != emk;
      epos = s_carry[0];
      emk = s_carry[1];
    }
    if (__syncthreads_or(dirty ? 1 : 0)) run_fixed_point(s, h, natural, chunk, im.nchunks, rec, epos, emk, lane, dirty, s_pos, s_mk);
    __syncthreads();   // (the records of this run are written before the next one reads its carry)
  }
  // exclusive scan over the chunks: blocks in front, predictors at the entry (counted from the last reset)
  const int per = (im.nchunks + kThreads - 1) / kThreads;
  const int c0 = t * per, c1 = min(c0 + per, im.nchunks);
  int acc[5] = {0, 0, 0, 0, 0};
  for (int c = c0; c < c1; ++c) {
    const int* r = rec + (int64_t)c * kRecInts;
    acc[0] += r[4];
    if (r[5]) {
      acc[1] = 1;
      acc[2] = acc[3] = acc[4] = 0;
    }
    for (int k = 0; k < 3; ++k) acc[2 + k] = (int)((unsigned)acc[2 + k] + (unsigned)r[6 + k]);
  }
  for (int k = 0; k < 5; ++k) s_sum[t][k] = acc[k];
  __syncthreads();
  if (t == 0) {
    int run5[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < kThreads; ++i) {
      int mine[5];
      for (int k = 0; k < 5; ++k) {
        mine[k] = s_sum[i][k];
        s_sum[i][k] = run5[k];
      }
      run5[0] += mine[0];
      for (int k = 2; k < 5; ++k) run5[k] = mine[1] ? mine[k] : (int)((unsigned)run5[k] + (unsigned)mine[k]);
    }
  }
  __syncthreads();
  int blocks = s_sum[t][0], pred[3] = {s_sum[t][2], s_sum[t][3], s_sum[t][4]};
  for (int c = c0; c < c1; ++c) {
    int* r = rec + (int64_t)c * kRecInts;
    r[9] = blocks;
    r[10] = pred[0];
    r[11] = pred[1];
    r[12] = pred[2];
    blocks += r[4];
    for (int k = 0; k < 3; ++k) pred[k] = r[5] ? r[6 + k] : (int)((unsigned)pred[k] + (unsigned)r[6 + k]);
  }
}

__global__ __launch_bounds__(kThreads) void jpegdec_coefficients(DecTable tab, const unsigned char* scans, const unsigned char* tables,
                                                                  unsigned char* ws, unsigned* keys) {
  __shared__ Huff h;
  __shared__ unsigned char natural[64];
  const DecImage& im = tab.img[blockIdx.y];
  if ((int)blockIdx.x * kRun >= im.nchunks) return;
  Scan s;
  load_tables(im, tables + (int64_t)blockIdx.y * CODETR_JPEGDEC_TABLE_BYTES, &h, natural, &s, scans);
  const int chunk = blockIdx.x * kRun + threadIdx.x;
  if (chunk >= im.nchunks) return;
  const int* r = reinterpret_cast<const int*>(ws + im.rec_off) + (int64_t)chunk * kRecInts;
  const int pred[3] = {r[10], r[11], r[12]};
  const int first = r[9] < 0 ? 0 : r[9];
  const int chunk_end = chunk == im.nchunks - 1 ? 0x7FFFFFFF : (chunk + 1) * kChunk;
  Lane lane;
  decode_chunk<true>(s, h, natural, r[0], r[1], chunk * kChunk, chunk_end, first, pred, reinterpret_cast<short*>(ws + im.coef_off), &lane);
  if (lane.err) atomicMin(&keys[blockIdx.y], ((unsigned)chunk << 4) | (unsigned)lane.err);   // the first in scan order
}

__global__ __launch_bounds__(kIdctBlocks * 8) void jpegdec_idct(DecTable tab, const unsigned char* tables, unsigned char* ws) {
  __shared__ int32_t mid[kIdctBlocks][64];
  const DecImage& im = tab.img[blockIdx.y];
  if ((int64_t)blockIdx.x * kIdctBlocks >= im.nblocks) return;
  const int j = threadIdx.x >> 3, l = threadIdx.x & 7;
  const int g = blockIdx.x * kIdctBlocks + j;
  const bool valid = g < im.nblocks;
  int comp = 0, bx = 0, by = 0;
  if (valid) {
    const int mcu = g / im.bpm, i = g % im.bpm, my = mcu / im.mcus_x, mx = mcu % im.mcus_x;
    if (im.ncomp == 1 || i < im.bpm - 2) {
      bx = mx * im.hmax + (im.ncomp == 1 ? 0 : i % im.hmax);
      by = my * im.vmax + (im.ncomp == 1 ? 0 : i / im.hmax);
    } else {
      comp = i - (im.bpm - 2) + 1;
      bx = mx;
      by = my;
    }
    const short* coef = reinterpret_cast<const short*>(ws + im.coef_off) + (int64_t)g * 64;
    const unsigned char* q = tables + (int64_t)blockIdx.y * CODETR_JPEGDEC_TABLE_BYTES + (im.tq[comp] & 3) * 64;
    int32_t v[8];
#pragma unroll
    for (int i2 = 0; i2 < 8; ++i2) v[i2] = (int32_t)((uint32_t)(int32_t)coef[8 * i2 + l] * (uint32_t)q[8 * i2 + l]);
    idct_1d(v, 1, &mid[j][l], 8, 11);
  }
  __syncthreads();
  if (valid) {
    int bw, bh;
    int64_t off;
    plane_of(im, comp, &bw, &bh, &off);
    int32_t v[8], o[8];
#pragma unroll
    for (int i2 = 0; i2 < 8; ++i2) v[i2] = mid[j][8 * l + i2];
    idct_1d(v, 1, o, 1, 18);
    unsigned char* dst = ws + im.plane_off + off + ((int64_t)by * 8 + l) * ((int64_t)bw * 8) + bx * 8;
#pragma unroll
    for (int i2 = 0; i2 < 8; ++i2) dst[i2] = (unsigned char)clamp255(o[i2] + 128);
  }
}

__global__ __launch_bounds__(256) void jpegdec_pixels(DecTable tab, const unsigned char* ws, unsigned char* dst, const unsigned* keys,
                                                       int* status) {
  const DecImage& im = tab.img[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) status[blockIdx.y] = keys[blockIdx.y] == 0xFFFFFFFFu ? 0 : (int)(keys[blockIdx.y] & 15u);
  if (i >= (int64_t)im.H * im.W) return;
  const int y = (int)(i / im.W), x = (int)(i % im.W);
  int bw, bh;
  int64_t off;
  plane_of(im, 0, &bw, &bh, &off);
  const int Y = ws[im.plane_off + (int64_t)y * bw * 8 + x];
  unsigned char* out = dst + im.dst_off + i * 3;
  if (im.ncomp == 1) {
    out[0] = out[1] = out[2] = (unsigned char)Y;
    return;
  }
  const int dw = (im.W + im.hmax - 1) / im.hmax, dh = (im.H + im.vmax - 1) / im.vmax;
  int c[2];
  for (int k = 0; k < 2; ++k) {
    plane_of(im, 1 + k, &bw, &bh, &off);
    c[k] = upsample(ws + im.plane_off + off, (int64_t)bw * 8, dw, dh, im.hmax, im.vmax, x, y);
  }
  ycc_to_rgb(Y, c[0], c[1], out);
}

// the checks and the workspace layout: keys [N] (16-byte rounded), records, coefficients, planes
int64_t plan(int64_t N, const int64_t* rows, const int32_t* infos, int64_t scans_bytes, int64_t dst_bytes, DecTable* tab,
             int64_t* coef_off, int64_t* coef_bytes, int* max_runs, int* max_blocks, int64_t* max_pixels) {
  if (!rows || !infos || N <= 0) return CODETR_E_BADARG;
  if (N > CODETR_PREPROCESS_BATCH_MAX) return CODETR_E_TOO_LARGE;
  int64_t rec = 0, coef = 0, planes = 0;
  for (int64_t n = 0; n < N; ++n) {
    const int64_t* r = rows + CODETR_JPEGDEC_ROW_INTS * n;
    const int32_t* in = infos + CODETR_JPEGDEC_INFO_INTS * n;
    const int64_t H = r[2], W = r[3];
    if (r[0] < 0 || r[1] < 0 || r[4] < 0 || H <= 0 || W <= 0) return CODETR_E_BADARG;
    if (H > CODETR_FRAME_MAX_SIDE || W > CODETR_FRAME_MAX_SIDE || r[1] > CODETR_JPEGDEC_MAX_FILE_BYTES) return CODETR_E_TOO_LARGE;
    if (in[0] != H || in[1] != W || in[5] != r[1]) return CODETR_E_BADARG;
    if (in[6] != 0) return CODETR_E_UNSUPPORTED;
    const int nc = in[2], hm = in[7], vm = in[8];
    if (nc != 1 && nc != 3) return CODETR_E_UNSUPPORTED;
    if (nc == 1 ? (hm != 1 || vm != 1) : !((hm == 1 && vm == 1) || (hm == 2 && vm == 1) || (hm == 2 && vm == 2)))
      return CODETR_E_UNSUPPORTED;
    const int64_t mx = (W + 8 * hm - 1) / (8 * hm), my = (H + 8 * vm - 1) / (8 * vm), bpm = nc == 1 ? 1 : hm * vm + 2;
    if (in[24] != mx || in[25] != my || in[26] != bpm || in[27] != mx * my * bpm || in[3] < 0 || in[3] > 65535)
      return CODETR_E_BADARG;
    for (int c = 0; c < nc; ++c) {
      if (in[9 + 5 * c] != (c ? 1 : hm) || in[10 + 5 * c] != (c ? 1 : vm)) return CODETR_E_BADARG;
      for (int k = 11; k < 14; ++k)
        if (in[k + 5 * c] < 0 || in[k + 5 * c] > 3) return CODETR_E_BADARG;
    }
    if (scans_bytes >= 0 && (r[0] > scans_bytes || r[1] > scans_bytes - r[0])) return CODETR_E_BADARG;
    if (dst_bytes >= 0 && (r[4] > dst_bytes || H * W * 3 > dst_bytes - r[4])) return CODETR_E_BADARG;
    for (int64_t m = 0; m < n && dst_bytes >= 0; ++m) {   // the images are written: they must not overlap
      const int64_t* o = rows + CODETR_JPEGDEC_ROW_INTS * m;
      if (r[4] < o[4] + o[2] * o[3] * 3 && o[4] < r[4] + H * W * 3) return CODETR_E_BADARG;
    }
    const int64_t chunks = r[1] / kChunk + 1;   // (an empty scan still has one chunk: its lane reports the exhaustion)
    const int64_t runs = (chunks + kRun - 1) / kRun;
    if (tab) {
      DecImage& im = tab->img[n];
      im.scan_off = r[0];
      im.dst_off = r[4];
      im.rec_off = rec;          // (offsets within their regions; the caller adds the regions' starts)
      im.coef_off = coef;
      im.plane_off = planes;
      im.H = (int)H;
      im.W = (int)W;
      im.scan_len = (int)r[1];
      im.dri = in[3];
      im.nchunks = (int)chunks;
      im.mcus_x = (int)mx;
      im.mcus_y = (int)my;
      im.nblocks = in[27];
      im.ncomp = (unsigned char)nc;
      im.bpm = (unsigned char)bpm;
      im.hmax = (unsigned char)hm;
      im.vmax = (unsigned char)vm;
      for (int c = 0; c < 3; ++c) {
        im.tq[c] = (unsigned char)(c < nc ? in[11 + 5 * c] : 0);
        im.td[c] = (unsigned char)(c < nc ? in[12 + 5 * c] : 0);
        im.ta[c] = (unsigned char)(c < nc ? in[13 + 5 * c] : 0);
      }
      if (runs > *max_runs) *max_runs = (int)runs;
      if (in[27] > *max_blocks) *max_blocks = in[27];
      if (H * W > *max_pixels) *max_pixels = H * W;
    }
    rec += runs * kRun * kRecInts * 4;
    coef += (int64_t)in[27] * 128;
    planes += ((int64_t)in[27] * 64 + 15) / 16 * 16;
  }
  const int64_t keys = (N * 4 + 15) / 16 * 16;
  if (tab) {
    for (int64_t n = 0; n < N; ++n) {
      tab->img[n].rec_off += keys;
      tab->img[n].coef_off += keys + rec;
      tab->img[n].plane_off += keys + rec + coef;
    }
    *coef_off = keys + rec;
    *coef_bytes = coef;
  }
  return keys + rec + coef + planes;
}

}  // namespace

extern "C" {

int codetr_jpegdec_abi_version(void) { return CODETR_JPEGDEC_ABI_VERSION; }

int codetr_jpegdec_parse(const unsigned char* file_host, int64_t bytes, int32_t* info_host, unsigned char* tables_host) {
  return jpegdec::parse(file_host, bytes, info_host, tables_host);
}

int64_t codetr_jpegdec_output_bytes(int64_t H, int64_t W) {
  if (H < 1 || W < 1) return CODETR_E_BADARG;
  if (H > CODETR_FRAME_MAX_SIDE || W > CODETR_FRAME_MAX_SIDE) return CODETR_E_TOO_LARGE;
  return (H * W * 3 + 15) / 16 * 16;
}

int64_t codetr_jpegdec_workspace_bytes(int64_t N, const int64_t* rows_host, const int32_t* infos_host) {
  return plan(N, rows_host, infos_host, -1, -1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int codetr_jpegdec_decode_u8(void* stream, const void* scans_dev, int64_t scans_bytes, int64_t N, const int64_t* rows_host,
                             const int32_t* infos_host, const void* tables_dev, void* dst_dev, int64_t dst_bytes, int* status_dev,
                             void* workspace_dev, int64_t workspace_bytes) {
  if (!scans_dev || !rows_host || !infos_host || !tables_dev || !dst_dev || !status_dev || !workspace_dev || scans_bytes < 0 ||
      dst_bytes <= 0)
    return CODETR_E_BADARG;
  DecTable tab = {};
  int64_t coef_off = 0, coef_bytes = 0, max_pixels = 0;
  int max_runs = 0, max_blocks = 0;
  const int64_t need = plan(N, rows_host, infos_host, scans_bytes, dst_bytes, &tab, &coef_off, &coef_bytes, &max_runs, &max_blocks,
                            &max_pixels);
  if (need < 0) return (int)need;
  if (workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace_dev) & 15u)) return CODETR_E_BADARG;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace_dev);
  const unsigned char* scans = static_cast<const unsigned char*>(scans_dev);
  const unsigned char* tables = static_cast<const unsigned char*>(tables_dev);
  unsigned* keys = reinterpret_cast<unsigned*>(ws);
  hipError_t err = hipMemsetAsync(keys, 0xFF, (size_t)N * 4, s);
  if (err != hipSuccess) return (int)err;
  err = hipMemsetAsync(ws + coef_off, 0, (size_t)coef_bytes, s);
  if (err != hipSuccess) return (int)err;
  hipLaunchKernelGGL(jpegdec_sync_runs, dim3((unsigned)max_runs, (unsigned)N), dim3(kThreads), 0, s, tab, scans, tables, ws);
  if ((err = hipGetLastError()) != hipSuccess) return (int)err;
  hipLaunchKernelGGL(jpegdec_link_runs, dim3((unsigned)N), dim3(kThreads), 0, s, tab, scans, tables, ws);
  if ((err = hipGetLastError()) != hipSuccess) return (int)err;
  hipLaunchKernelGGL(jpegdec_coefficients, dim3((unsigned)max_runs, (unsigned)N), dim3(kThreads), 0, s, tab, scans, tables, ws, keys);
  if ((err = hipGetLastError()) != hipSuccess) return (int)err;
  hipLaunchKernelGGL(jpegdec_idct, dim3((unsigned)((max_blocks + kIdctBlocks - 1) / kIdctBlocks), (unsigned)N), dim3(kIdctBlocks * 8),
                     0, s, tab, tables, ws);
  if ((err = hipGetLastError()) != hipSuccess) return (int)err;
  hipLaunchKernelGGL(jpegdec_pixels, dim3((unsigned)((max_pixels + 255) / 256), (unsigned)N), dim3(256), 0, s, tab, ws,
                     static_cast<unsigned char*>(dst_dev), keys, status_dev);
  err = hipGetLastError();
  return err == hipSuccess ? 0 : (int)err;
}

}  // extern "C"
