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

// ---- The split plan (csrc/jpeg_split.hip): items too long for one wavefront are cut into sub-sequences of `subseq_bytes`
// UNSTUFFED bytes that 256-lane workgroups decode in parallel.  The number of unstuffed bytes is known only on the device, so
// the count comes from the stuffed length, an upper bound: n_sub = ceil(len / subseq_bytes); sub-sequences behind the last
// unstuffed byte are empty.  Split is the layout of mr_jpeg_split; every offset is into the workspace and 16-byte aligned.
struct Split {
  int item, image;                // the work item (items[item].reserved = 1 + this entry's index) and its image
  int subseq_bytes, n_sub, n_wg;  // n_wg = ceil(n_sub / 256) workgroups
  int n_blocks;                   // nmcu * B blocks wanted, B = hs * vs + 2 (colour) or 1 (gray)
  int blocks_per_mcu, reserved;
  long long meta_off;             // int [4]: unstuffed bytes, blocks completed, 0, 0
  long long raw_off, raw_bytes;   // the unstuffed bytes, zero behind the last one up to raw_bytes
  long long in_off, exit_off;     // per sub-sequence, 8 bytes each: the state it was decoded from / the state it produced
  long long wg_exit_off;          // [2][n_wg] x 8 bytes: the exit state of each workgroup, one copy per pass parity
  long long block_off;            // int [n_sub]: blocks completed in front of each sub-sequence
  long long coef_off, coef_bytes; // int dc[n_blocks], then short coef[n_blocks][64] in zigzag order (zeroed by the decoder)
};

constexpr int SPLIT_WG = 256;                       // sub-sequences per workgroup
constexpr long long SPLIT_MAX_LEN = 1LL << 27;      // bit positions stay below 2^31

static inline bool split_wanted(const Image* images, const Item& it, long long split_above) {
  return it.reserved == 0 && images[it.image].status == OK && it.len > split_above && it.len > 0 && it.len < SPLIT_MAX_LEN &&
         it.nmcu > 0;
}

// Describes every item longer than `split_above` bytes in splits[] and appends its regions to *workspace_bytes.  Returns the
// number of such items; when that exceeds max_splits NOTHING is written (call again with room).  subseq_bytes: a multiple of 4
// in [16, 1024] (the caller checks).
static inline long long plan_split(const Image* images, Item* items, long long n_items, long long split_above, int subseq_bytes,
                                   Split* splits, long long max_splits, long long* workspace_bytes) {
  long long count = 0;
  for (long long i = 0; i < n_items; ++i) count += split_wanted(images, items[i], split_above) ? 1 : 0;
  if (count > max_splits) return count;
  long long ws = align16(*workspace_bytes), k = 0;
  auto take = [&ws](long long bytes) {
    const long long at = ws;
    ws = align16(ws + bytes);
    return at;
  };
  for (long long i = 0; i < n_items; ++i) {
    if (!split_wanted(images, items[i], split_above)) continue;
    const Image& im = images[items[i].image];
    Split s;
    memset(&s, 0, sizeof(s));
    s.item = (int)i, s.image = items[i].image;
    s.subseq_bytes = subseq_bytes;
    s.n_sub = (int)((items[i].len + subseq_bytes - 1) / subseq_bytes);
    s.n_wg = (s.n_sub + SPLIT_WG - 1) / SPLIT_WG;
    s.blocks_per_mcu = im.ncomp == 3 ? im.hs * im.vs + 2 : 1;
    s.n_blocks = items[i].nmcu * s.blocks_per_mcu;
    s.meta_off = take(16);
    s.raw_bytes = align16((long long)s.n_sub * subseq_bytes) + 16;
    s.raw_off = take(s.raw_bytes);
    s.in_off = take(8LL * s.n_sub);
    s.exit_off = take(8LL * s.n_sub);
    s.wg_exit_off = take(16LL * s.n_wg);
    s.block_off = take(4LL * s.n_sub);
    s.coef_bytes = align16(4LL * s.n_blocks) + 128LL * s.n_blocks;
    s.coef_off = take(s.coef_bytes);
    items[i].reserved = (int)k + 1;
    splits[k++] = s;
  }
  *workspace_bytes = ws;
  return count;
}

}  // namespace jpeg
}  // namespace mr
