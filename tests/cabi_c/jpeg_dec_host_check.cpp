// Host memory check of the JPEG decoder: the header parser (csrc/jpeg_dec_parse.h) and the decoder core the kernels call
// (csrc/jpeg_dec_core.h), compiled for the host and run as a stand-alone program under -fsanitize=address,undefined:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Ico-detr-tensorrt_amd/csrc
//       tests/cabi_c/jpeg_dec_host_check.cpp -o jpeg_dec_host_check
//   ./jpeg_dec_host_check [--out DIR] [--corrupt K] FILE.jpg ...
// Per file: the parser on the whole file and on its prefixes (every one that cuts the header); when the file is supported, the chunked decode as the
// kernels run it (the same lanes, chunk bounds, block-count guards and plane sizes, one lane after the other), and K
// seeded corruptions of the scan bytes through the same loop.  Every buffer is a heap block of exactly the size the
// kernels are promised, so the sanitizer sees any access outside it.  Prints `name rc reason status` per file and, with
// --out, writes DIR/name.rgb (H x W x 3) for the tests to compare with the restatement.  Exit status 0 when nothing is out
// of range and every decode ended with a status from the header.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "jpeg_dec_core.h"
#include "jpeg_dec_parse.h"

using namespace jpegdec;

namespace {

struct Rec {
  int epos, emk;
  Lane lane;
};

struct Rng {   // xorshift32: the corruptions are the same on every machine
  uint32_t s;
  uint32_t next() {
    s ^= s << 13;
    s ^= s >> 17;
    s ^= s << 5;
    return s;
  }
};

// the five launches of csrc/jpeg_dec.hip, lane after lane; rgb may be null
int decode(const int32_t* info, const unsigned char* tables, const unsigned char* scan_bytes, int len, std::vector<unsigned char>* rgb) {
  std::vector<unsigned char> scan(scan_bytes, scan_bytes + len);   // exactly len bytes
  Huff h;
  for (int t = 0; t < 8; ++t) huff_build(tables + kQuantBytes + t * kHuffBytes, t, &h);
  const int H = info[0], W = info[1], nc = info[2], hm = info[7], vm = info[8], mx = info[24], my = info[25], bpm = info[26];
  Scan s;
  s.data = scan.data();
  s.len = len;
  s.dri = info[3];
  s.bpm = bpm;
  s.nblocks = info[27];
  for (int i = 0; i < 6; ++i) s.comp[i] = (unsigned char)(nc == 1 ? 0 : (i < bpm - 2 ? 0 : i - (bpm - 2) + 1));
  for (int c = 0; c < 3; ++c) {
    s.td[c] = (unsigned char)(c < nc ? info[12 + 5 * c] : 0);
    s.ta[c] = (unsigned char)(c < nc ? info[13 + 5 * c] : 0);
  }
  const int nchunks = len / kChunk + 1;
  std::vector<Rec> rec((size_t)nchunks);
  auto end_of = [&](int c) { return c == nchunks - 1 ? 0x7FFFFFFF : (c + 1) * kChunk; };
  auto fixed_point = [&](int c0, int c1, std::vector<int> dirty) {
    for (int round = 0; round <= kRun && !dirty.empty(); ++round) {
      for (int c : dirty) decode_chunk<false>(s, h, kNatural, rec[c].epos, rec[c].emk, c * kChunk, end_of(c), 0, nullptr, nullptr, &rec[c].lane);
      std::vector<int> again;
      for (int c = c0 + 1; c < c1; ++c)
        if (rec[c - 1].lane.pos != rec[c].epos || rec[c - 1].lane.mk != rec[c].emk) {
          rec[c].epos = rec[c - 1].lane.pos;
          rec[c].emk = rec[c - 1].lane.mk;
          again.push_back(c);
        }
      dirty.swap(again);
    }
    return dirty.empty();
  };
  for (int c = 0; c < nchunks; ++c) rec[c].epos = c * kChunk * 8, rec[c].emk = 0;
  for (int c0 = 0; c0 < nchunks; c0 += kRun) {
    std::vector<int> all;
    const int c1 = c0 + kRun < nchunks ? c0 + kRun : nchunks;
    for (int c = c0; c < c1; ++c) all.push_back(c);
    if (!fixed_point(c0, c1, all)) return -100;   // the fixed point must settle within a round per chunk
  }
  for (int c0 = kRun; c0 < nchunks; c0 += kRun)
    if (rec[c0 - 1].lane.pos != rec[c0].epos || rec[c0 - 1].lane.mk != rec[c0].emk) {
      rec[c0].epos = rec[c0 - 1].lane.pos;
      rec[c0].emk = rec[c0 - 1].lane.mk;
      if (!fixed_point(c0, c0 + kRun < nchunks ? c0 + kRun : nchunks, std::vector<int>(1, c0))) return -100;
    }
  std::vector<short> coef((size_t)s.nblocks * 64, 0);
  unsigned key = 0xFFFFFFFFu;
  int blocks = 0, pred[3] = {0, 0, 0};
  for (int c = 0; c < nchunks; ++c) {
    Lane lane;
    decode_chunk<true>(s, h, kNatural, rec[c].epos, rec[c].emk, c * kChunk, end_of(c), blocks, pred, coef.data(), &lane);
    if (lane.pos != rec[c].lane.pos || lane.mk != rec[c].lane.mk || lane.nblk != rec[c].lane.nblk) return -101;
    if (lane.err) {
      const unsigned k = ((unsigned)c << 4) | (unsigned)lane.err;
      if (k < key) key = k;
    }
    blocks += rec[c].lane.nblk;
    for (int k = 0; k < 3; ++k) pred[k] = rec[c].lane.reset ? rec[c].lane.dc[k] : (int)((unsigned)pred[k] + (unsigned)rec[c].lane.dc[k]);
  }
  const int status = key == 0xFFFFFFFFu ? 0 : (int)(key & 15u);
  // planes: Y over mx * hm x my * vm blocks, then Cb, Cr over mx x my
  const int64_t y_bytes = (int64_t)mx * hm * my * vm * 64, c_bytes = (int64_t)mx * my * 64;
  std::vector<unsigned char> planes((size_t)s.nblocks * 64);
  for (int g = 0; g < s.nblocks; ++g) {
    const int mcu = g / bpm, i = g % bpm, yy = mcu / mx, xx = mcu % mx;
    int comp = 0, bx, by, bw = mx * hm;
    if (nc == 1 || i < bpm - 2) {
      bx = xx * hm + (nc == 1 ? 0 : i % hm);
      by = yy * vm + (nc == 1 ? 0 : i / hm);
    } else {
      comp = i - (bpm - 2) + 1;
      bx = xx;
      by = yy;
      bw = mx;
    }
    unsigned char* base = planes.data() + (comp == 0 ? 0 : y_bytes + (comp - 1) * c_bytes);
    idct_block(coef.data() + (size_t)g * 64, tables + (info[11 + 5 * comp] & 3) * 64, base + ((int64_t)by * 8) * (bw * 8) + bx * 8, (int64_t)bw * 8);
  }
  if (rgb) {
    rgb->assign((size_t)H * W * 3, 0);
    const int dw = (W + hm - 1) / hm, dh = (H + vm - 1) / vm;
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        unsigned char* out = rgb->data() + ((size_t)y * W + x) * 3;
        const int Y = planes[(size_t)y * mx * hm * 8 + x];
        if (nc == 1) {
          out[0] = out[1] = out[2] = (unsigned char)Y;
          continue;
        }
        const int cb = upsample(planes.data() + y_bytes, (int64_t)mx * 8, dw, dh, hm, vm, x, y);
        const int cr = upsample(planes.data() + y_bytes + c_bytes, (int64_t)mx * 8, dw, dh, hm, vm, x, y);
        ycc_to_rgb(Y, cb, cr, out);
      }
  }
  return status;
}

}  // namespace

int main(int argc, char** argv) {
  std::string out_dir;
  int corrupt = 300, failures = 0;
  std::vector<std::string> files;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--out") && i + 1 < argc) out_dir = argv[++i];
    else if (!strcmp(argv[i], "--corrupt") && i + 1 < argc) corrupt = atoi(argv[++i]);
    else files.push_back(argv[i]);
  }
  for (const std::string& path : files) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) {
      fprintf(stderr, "cannot open %s\n", path.c_str());
      return 2;
    }
    std::vector<unsigned char> data;
    unsigned char buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) data.insert(data.end(), buf, buf + n);
    fclose(f);
    const size_t slash = path.find_last_of('/');
    const std::string name = slash == std::string::npos ? path : path.substr(slash + 1);
    int32_t info[CODETR_JPEGDEC_INFO_INTS];
    std::vector<unsigned char> tables(CODETR_JPEGDEC_TABLE_BYTES);
    const int rc = parse(data.data(), (int64_t)data.size(), info, tables.data());
    // every prefix that cuts the header (and a little of the scan), then every 509th: each in a block of its own size
    const size_t dense = rc == 0 ? (size_t)info[4] + 64 : data.size();
    for (size_t n = 0; n < data.size(); n += n < dense ? 1 : 509) {
      std::vector<unsigned char> prefix(data.begin(), data.begin() + n);
      int32_t pi[CODETR_JPEGDEC_INFO_INTS];
      std::vector<unsigned char> pt(CODETR_JPEGDEC_TABLE_BYTES);
      const int prc = parse(prefix.data(), (int64_t)n, pi, pt.data());
      if (prc == 0 && (pi[4] < 0 || pi[5] < 0 || (size_t)pi[4] + (size_t)pi[5] > n)) {
        printf("%s: prefix %zu parses to a scan outside it\n", name.c_str(), n);
        ++failures;
      } else if (prc != 0 && prc != CODETR_E_BADARG && prc != CODETR_E_UNSUPPORTED && prc != CODETR_E_TOO_LARGE) {
        printf("%s: prefix %zu returns %d\n", name.c_str(), n, prc);
        ++failures;
      }
    }
    int status = -1;
    if (rc == 0) {
      std::vector<unsigned char> rgb;
      status = decode(info, tables.data(), data.data() + info[4], info[5], &rgb);
      if (status < 0 || status > CODETR_JPEGDEC_S_INTERVAL) ++failures;
      if (!out_dir.empty()) {
        FILE* o = fopen((out_dir + "/" + name + ".rgb").c_str(), "wb");
        if (!o || fwrite(rgb.data(), 1, rgb.size(), o) != rgb.size()) {
          fprintf(stderr, "cannot write to %s\n", out_dir.c_str());
          return 2;
        }
        fclose(o);
      }
      Rng rng = {0x9E3779B9u ^ (uint32_t)data.size()};
      int with_status = 0;
      for (int k = 0; k < corrupt && info[5] > 0; ++k) {
        std::vector<unsigned char> scan(data.begin() + info[4], data.begin() + info[4] + info[5]);
        const int kind = k % 4;
        if (kind == 0) {   // bit flips
          for (int j = 0, n = 1 + (int)(rng.next() % 4); j < n; ++j) scan[rng.next() % scan.size()] ^= (unsigned char)(1u << (rng.next() % 8));
        } else if (kind == 1) {   // a cut scan
          scan.resize(rng.next() % scan.size());
        } else if (kind == 2) {   // random bytes, markers among them
          for (int j = 0, n = 1 + (int)(rng.next() % 3); j < n; ++j) {
            const size_t at = rng.next() % scan.size();
            scan[at] = (rng.next() & 1) ? 0xFF : (unsigned char)rng.next();
            if (at + 1 < scan.size() && (rng.next() & 1)) scan[at + 1] = (unsigned char)(0xD0 + rng.next() % 16);
          }
        } else {   // a run of one value
          const size_t at = rng.next() % scan.size(), n = 1 + rng.next() % 40;
          const unsigned char v = (rng.next() & 1) ? 0xFF : 0x00;
          for (size_t j = at; j < at + n && j < scan.size(); ++j) scan[j] = v;
        }
        const int st = decode(info, tables.data(), scan.data(), (int)scan.size(), nullptr);
        if (st < 0 || st > CODETR_JPEGDEC_S_INTERVAL) {
          printf("%s: corruption %d ends with %d\n", name.c_str(), k, st);
          ++failures;
        }
        with_status += st != 0;
      }
      printf("%s %d %d %d corrupt %d/%d\n", name.c_str(), rc, info[6], status, with_status, corrupt);
    } else {
      printf("%s %d %d %d\n", name.c_str(), rc, info[6], status);
    }
  }
  printf("%s\n", failures ? "FAILED" : "clean");
  return failures ? 1 : 0;
}
