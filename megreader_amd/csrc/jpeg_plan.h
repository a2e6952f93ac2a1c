// Host plan of the GPU JPEG decoder (csrc/jpeg.hip, include/megreader_hip.h: mr_jpeg_plan): the marker parser.  Plain C++ with
// no HIP and no allocation, so that a stand-alone program can drive it under the host sanitizers (tools/check_jpeg_plan.cpp).
//
// One pass over the marker segments of each blob (ITU-T T.81 B.2) fills one `Image` -- shape, sampling, the quantisation tables
// and the canonical Huffman tables (C.2: per-length largest code and symbol offset, up to 256 symbols) -- and a byte scan of the
// entropy-coded segment cuts it into work items at the RSTn markers: DC predictors reset there (E.2.4), so the items decode
// independently, one wavefront each.  Every length and index read from the file is checked against the blob and the table sizes
// before it is used; whatever the device cannot decode is marked UNSUPPORTED (the caller decodes it on the host), whatever
// contradicts the syntax CORRUPT, and only an OK image gets offsets.
//
// Image and Item are the layouts of mr_jpeg_image / mr_jpeg_item of the C header, restated here because that header includes
// the HIP runtime's; csrc/jpeg.hip asserts that the two agree.
#pragma once
#include <string.h>

namespace mr {
namespace jpeg {

enum { OK = 0, UNSUPPORTED = 1, CORRUPT = 2 };

struct Image {
  int status, h, w, ncomp;
  int hs, vs;                  // luma sampling factors (chroma is 1x1)
  int mcu_w, mcu_h;            // MCUs per row, MCU rows
  int restart;                 // restart interval in MCUs, 0: none
  int first_item, n_items;
  int reserved0;
  long long blob_off, blob_len;   // the blob inside the staged blob buffer (16-byte aligned)
  long long scan_off, scan_len;   // the entropy-coded segment inside the blob
  long long plane_off[3];         // component planes inside the workspace, padded to whole MCUs
  int plane_pitch[3], plane_rows[3];
  long long out_off;              // first output byte; the image occupies h * w * 3 bytes from there
  int comp_tq[3], comp_td[3], comp_ta[3];
  int reserved1;
  int quant[64];                  // 4 tables x 64 bytes in memory order, zigzag order
  int huff_maxcode[64];           // [DC0, DC1, AC0, AC1][length - 1]: largest code of that length, -1: none
  int huff_valoff[64];            // same index: (index of the first symbol of that length) - (its code)
  int huff_sym[256];              // 4 tables x 256 bytes in memory order
};

struct Item {
  int image, mcu0, nmcu, reserved;
  long long off, len;             // stuffed bytes of these MCUs inside the blob; no marker inside
};

struct Totals {
  long long n_items, blob_bytes, workspace_bytes, out_bytes;
};

static inline long long align16(long long v) { return (v + 15) & ~15LL; }

// Everything of one image except the offsets into the shared buffers.  Items are appended at items[*n_items] while
// *n_items < max_items and counted beyond.  Returns the status (also stored in im->status).
static inline int parse_one(const unsigned char* b, long long n, int index, Image* im, Item* items, long long max_items,
                            long long* n_items) {
  memset(im, 0, sizeof(*im));
  im->blob_len = n;
#define MR_JPEG_FAIL(code) return im->status = (code)
  if (b == nullptr || n < 2 || b[0] != 0xFF || b[1] != 0xD8) MR_JPEG_FAIL(UNSUPPORTED);
  long long pos = 2;
  bool have_q[4] = {false, false, false, false}, have_h[4] = {false, false, false, false};
  bool frame = false, jfif = false, adobe = false;
  int transform = -1, cid[3] = {0, 0, 0}, chs[3] = {0, 0, 0}, cvs[3] = {0, 0, 0};
  unsigned char* quant = (unsigned char*)im->quant;
  unsigned char* sym = (unsigned char*)im->huff_sym;
  for (;;) {
    if (pos >= n || b[pos] != 0xFF) MR_JPEG_FAIL(CORRUPT);
    while (pos < n && b[pos] == 0xFF) ++pos;
    if (pos >= n) MR_JPEG_FAIL(CORRUPT);
    const int m = b[pos++];
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD8)) continue;
    if (m == 0xD9 || m == 0x00) MR_JPEG_FAIL(CORRUPT);
    if (pos + 2 > n) MR_JPEG_FAIL(CORRUPT);
    const long long L = b[pos] << 8 | b[pos + 1];
    if (L < 2 || pos + L > n) MR_JPEG_FAIL(CORRUPT);
    const unsigned char* seg = b + pos + 2;
    const long long sl = L - 2;
    if (m == 0xC0) {
      if (frame || sl < 6) MR_JPEG_FAIL(CORRUPT);
      const int prec = seg[0], h = seg[1] << 8 | seg[2], w = seg[3] << 8 | seg[4], nc = seg[5];
      if (prec != 8) MR_JPEG_FAIL(UNSUPPORTED);
      if (nc != 1 && nc != 3) MR_JPEG_FAIL(UNSUPPORTED);
      if (sl != 6 + 3 * nc || h == 0 || w == 0) MR_JPEG_FAIL(CORRUPT);
      for (int c = 0; c < nc; ++c) {
        const int tq = seg[8 + 3 * c];
        if (tq > 3) MR_JPEG_FAIL(CORRUPT);
        cid[c] = seg[6 + 3 * c];
        chs[c] = seg[7 + 3 * c] >> 4;
        cvs[c] = seg[7 + 3 * c] & 15;
        im->comp_tq[c] = tq;
      }
      im->h = h, im->w = w, im->ncomp = nc;
      frame = true;
    } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8) {
      MR_JPEG_FAIL(UNSUPPORTED);   // progressive, lossless, arithmetic, extended
    } else if (m == 0xDB) {
      for (long long i = 0; i < sl; i += 65) {
        const int pq = seg[i] >> 4, tq = seg[i] & 15;
        if (pq != 0) MR_JPEG_FAIL(pq == 1 ? UNSUPPORTED : CORRUPT);
        if (tq > 3 || i + 65 > sl) MR_JPEG_FAIL(CORRUPT);
        memcpy(quant + 64 * tq, seg + i + 1, 64);
        have_q[tq] = true;
      }
    } else if (m == 0xC4) {
      for (long long i = 0; i < sl;) {
        const int tc = seg[i] >> 4, th = seg[i] & 15;
        if (tc > 1 || th > 3 || i + 17 > sl) MR_JPEG_FAIL(CORRUPT);
        if (th > 1) MR_JPEG_FAIL(UNSUPPORTED);
        int total = 0;
        for (int l = 0; l < 16; ++l) total += seg[i + 1 + l];
        if (total > 256 || i + 17 + total > sl) MR_JPEG_FAIL(CORRUPT);
        const int t = tc * 2 + th;
        int code = 0, k = 0;
        for (int l = 1; l <= 16; ++l) {
          const int cnt = seg[i + l];
          im->huff_maxcode[t * 16 + l - 1] = -1;
          im->huff_valoff[t * 16 + l - 1] = 0;
          if (cnt) {
            im->huff_valoff[t * 16 + l - 1] = k - code;
            code += cnt;
            k += cnt;
            if (code > (1 << l)) MR_JPEG_FAIL(CORRUPT);
            im->huff_maxcode[t * 16 + l - 1] = code - 1;
          }
          code <<= 1;
        }
        memset(sym + 256 * t, 0, 256);
        memcpy(sym + 256 * t, seg + i + 17, (size_t)total);
        have_h[t] = true;
        i += 17 + total;
      }
    } else if (m == 0xDD) {
      if (L != 4) MR_JPEG_FAIL(CORRUPT);
      im->restart = seg[0] << 8 | seg[1];
    } else if (m == 0xE0) {
      if (sl >= 5 && memcmp(seg, "JFIF\0", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (sl >= 12 && memcmp(seg, "Adobe", 5) == 0) adobe = true, transform = seg[11];
    } else if (m == 0xDA) {
      if (!frame || sl < 1) MR_JPEG_FAIL(CORRUPT);
      const int ns = seg[0];
      if (ns < 1 || ns > 4 || sl != 4 + 2 * ns) MR_JPEG_FAIL(CORRUPT);
      if (ns != im->ncomp) MR_JPEG_FAIL(UNSUPPORTED);   // a scan per component: multi-scan
      for (int c = 0; c < ns; ++c) {
        const int t = seg[2 + 2 * c];
        if (seg[1 + 2 * c] != cid[c]) MR_JPEG_FAIL(UNSUPPORTED);
        if ((t >> 4) > 1 || (t & 15) > 1) MR_JPEG_FAIL(UNSUPPORTED);
        im->comp_td[c] = t >> 4;
        im->comp_ta[c] = t & 15;
      }
      if (seg[1 + 2 * ns] != 0 || seg[2 + 2 * ns] != 63 || seg[3 + 2 * ns] != 0) MR_JPEG_FAIL(UNSUPPORTED);
      for (int c = 0; c < ns; ++c)
        if (!have_q[im->comp_tq[c]] || !have_h[im->comp_td[c]] || !have_h[2 + im->comp_ta[c]]) MR_JPEG_FAIL(CORRUPT);
      pos += L;
      break;
    }
    pos += L;
  }
  if (im->ncomp == 3) {
    if (jfif) {
    } else if (adobe) {
      if (transform == 0) MR_JPEG_FAIL(UNSUPPORTED);   // RGB stored as is
    } else if (cid[0] == 82 && cid[1] == 71 && cid[2] == 66) {
      MR_JPEG_FAIL(UNSUPPORTED);                       // components named 'R', 'G', 'B'
    }
    const bool luma_ok = (chs[0] == 1 && cvs[0] == 1) || (chs[0] == 2 && cvs[0] == 1) || (chs[0] == 2 && cvs[0] == 2);
    if (!luma_ok || chs[1] != 1 || cvs[1] != 1 || chs[2] != 1 || cvs[2] != 1) MR_JPEG_FAIL(UNSUPPORTED);
    im->hs = chs[0], im->vs = cvs[0];
  } else {
    im->hs = im->vs = 1;   // a single-component scan is not interleaved: its sampling factors are moot
  }
  im->mcu_w = (im->w + 8 * im->hs - 1) / (8 * im->hs);
  im->mcu_h = (im->h + 8 * im->vs - 1) / (8 * im->vs);
  const long long total = (long long)im->mcu_w * im->mcu_h;
  const long long R = im->restart, want = R ? (total + R - 1) / R : 1;
  // the entropy-coded segment ends at the first marker that is neither a stuffed FF 00 nor RSTn, or with the blob
  im->scan_off = pos;
  im->first_item = (int)*n_items;
  long long start = pos, end = n, seen = 0;
  auto emit = [&](long long to) {
    if (seen < want) {
      if (*n_items < max_items) {
        Item& it = items[*n_items];
        it.image = index;
        it.mcu0 = (int)(seen * (R ? R : total));
        it.nmcu = (int)(R ? (total - seen * R < R ? total - seen * R : R) : total);
        it.reserved = 0;
        it.off = start;
        it.len = to - start;
      }
      ++*n_items;
    }
    ++seen;
  };
  bool bad = false;
  for (long long i = pos; i < n;) {
    if (b[i] != 0xFF) { ++i; continue; }
    long long j = i + 1;
    while (j < n && b[j] == 0xFF) ++j;   // fill bytes in front of a marker
    if (j >= n) { end = i; break; }
    if (b[j] == 0) { i = j + 1; continue; }
    if (b[j] >= 0xD0 && b[j] <= 0xD7) {
      if (R == 0 || b[j] - 0xD0 != (int)(seen & 7)) bad = true;
      emit(i);
      start = i = j + 1;
      continue;
    }
    end = i;
    break;
  }
  emit(end);
  im->scan_len = end - pos;
  im->n_items = (int)want;
  if (bad || seen != want) {
    *n_items = im->first_item;   // a failed image leaves no items
    MR_JPEG_FAIL(CORRUPT);
  }
#undef MR_JPEG_FAIL
  return im->status = OK;
}

// The whole batch: parse_one per blob, then the offsets.  Blobs are laid out back to back, each 16-byte aligned, in the order
// given (all of them, whatever their status: the caller stages one buffer); planes and output regions only for OK images, the
// output regions 16-byte aligned so that the colour kernel's 4-byte stores are.  `items` holds max_items entries; when
// totals->n_items exceeds that the list is incomplete and the call is to be repeated with room for all of them.
static inline void plan(int n, const void* const* blobs, const long long* lens, Image* images, Item* items, long long max_items,
                        Totals* totals) {
  Totals t = {0, 0, 0, 0};
  for (int i = 0; i < n; ++i) {
    Image* im = images + i;
    const long long len = lens[i] < 0 ? 0 : lens[i];
    parse_one((const unsigned char*)blobs[i], len, i, im, items, max_items, &t.n_items);
    im->blob_off = t.blob_bytes;
    t.blob_bytes = align16(t.blob_bytes + len);
    if (im->status != OK) continue;
    for (int c = 0; c < im->ncomp; ++c) {
      im->plane_pitch[c] = im->mcu_w * 8 * (c == 0 ? im->hs : 1);
      im->plane_rows[c] = im->mcu_h * 8 * (c == 0 ? im->vs : 1);
      im->plane_off[c] = t.workspace_bytes;
      t.workspace_bytes = align16(t.workspace_bytes + (long long)im->plane_pitch[c] * im->plane_rows[c]);
    }
    im->out_off = t.out_bytes;
    t.out_bytes = align16(t.out_bytes + (long long)im->h * im->w * 3);
  }
  *totals = t;
}

}  // namespace jpeg
}  // namespace mr
