// Stand-alone driver of the JPEG marker parser (megreader_amd/csrc/jpeg_plan.h) for the host sanitizers: no HIP, no Python.
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/check_jpeg_plan.cpp -o check_jpeg_plan
//   ./check_jpeg_plan tests/golden/jpeg/*.jpg
//
// For every file it plans (a) the file, (b) every prefix of it, (c) the file with each byte of its header (everything up to the
// entropy-coded segment) replaced by 0x00, 0xFF and its complement, and (d) all files as one batch.  Each blob is copied into an
// exactly-sized heap block so that a read past its end is a sanitizer report.  Wherever the plan says OK, every offset and length
// must lie inside the blob, the workspace and the output totals; the program exits non-zero otherwise.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../megreader_amd/csrc/jpeg_plan.h"

using namespace mr::jpeg;

static long long g_plans = 0, g_ok = 0;

static void fail(const char* what, const char* name, long long a, long long b) {
  fprintf(stderr, "FAIL %s: %s (%lld, %lld)\n", name, what, a, b);
  exit(1);
}

// The invariants of an OK plan for blobs of the given lengths.
static void verify(const char* name, int n, const long long* lens, const std::vector<Image>& images, const std::vector<Item>& items,
                   const Totals& t) {
  long long seen_items = 0;
  for (int i = 0; i < n; ++i) {
    const Image& im = images[i];
    if (im.blob_off < 0 || im.blob_off % 16 || im.blob_off + lens[i] > t.blob_bytes) fail("blob offset", name, i, im.blob_off);
    if (im.status != OK) continue;
    ++g_ok;
    if (im.h <= 0 || im.w <= 0 || (im.ncomp != 1 && im.ncomp != 3)) fail("shape", name, im.h, im.w);
    if (im.scan_off < 0 || im.scan_len < 0 || im.scan_off + im.scan_len > lens[i]) fail("scan range", name, im.scan_off, im.scan_len);
    for (int c = 0; c < im.ncomp; ++c) {
      const long long bytes = (long long)im.plane_pitch[c] * im.plane_rows[c];
      if (im.plane_off[c] < 0 || im.plane_off[c] % 16 || im.plane_off[c] + bytes > t.workspace_bytes)
        fail("plane offset", name, i, c);
      const int hs = c == 0 ? im.hs : 1, vs = c == 0 ? im.vs : 1;
      if (im.plane_pitch[c] != im.mcu_w * 8 * hs || im.plane_rows[c] != im.mcu_h * 8 * vs) fail("plane shape", name, i, c);
      if (im.plane_pitch[c] * (c == 0 ? 1 : im.hs) < im.w || im.plane_rows[c] * (c == 0 ? 1 : im.vs) < im.h)
        fail("plane smaller than the image", name, i, c);
      if (im.comp_tq[c] < 0 || im.comp_tq[c] > 3 || im.comp_td[c] < 0 || im.comp_td[c] > 1 || im.comp_ta[c] < 0 || im.comp_ta[c] > 1)
        fail("table selector", name, i, c);
    }
    if (im.out_off < 0 || im.out_off % 16 || im.out_off + (long long)im.h * im.w * 3 > t.out_bytes) fail("output offset", name, i, 0);
    if (im.first_item != seen_items || im.n_items < 1) fail("item range", name, im.first_item, im.n_items);
    long long mcu = 0;
    for (int k = 0; k < im.n_items; ++k) {
      if (im.first_item + k >= (long long)items.size()) fail("item list too short", name, i, k);
      const Item& it = items[im.first_item + k];
      if (it.image != i || it.mcu0 != mcu || it.nmcu < 1) fail("item MCUs", name, it.mcu0, it.nmcu);
      if (it.off < im.scan_off || it.len < 0 || it.off + it.len > im.scan_off + im.scan_len) fail("item bytes", name, it.off, it.len);
      mcu += it.nmcu;
    }
    if (mcu != (long long)im.mcu_w * im.mcu_h) fail("items do not cover the image", name, mcu, 0);
    seen_items += im.n_items;
  }
  if (seen_items != t.n_items) fail("item total", name, seen_items, t.n_items);
}

static void plan_batch(const char* name, const std::vector<std::vector<unsigned char>>& blobs) {
  const int n = (int)blobs.size();
  std::vector<unsigned char*> exact(n);
  std::vector<const void*> ptrs(n);
  std::vector<long long> lens(n);
  for (int i = 0; i < n; ++i) {
    lens[i] = (long long)blobs[i].size();
    exact[i] = (unsigned char*)malloc(blobs[i].size() ? blobs[i].size() : 1);   // exactly sized: one byte further is a report
    if (!blobs[i].empty()) memcpy(exact[i], blobs[i].data(), blobs[i].size());
    ptrs[i] = blobs[i].empty() ? nullptr : exact[i];
  }
  std::vector<Image> images(n);
  std::vector<Item> items(4);
  Totals t;
  plan(n, ptrs.data(), lens.data(), images.data(), items.data(), (long long)items.size(), &t);
  if (t.n_items > (long long)items.size()) {   // the documented second call
    items.resize((size_t)t.n_items);
    plan(n, ptrs.data(), lens.data(), images.data(), items.data(), (long long)items.size(), &t);
  }
  ++g_plans;
  verify(name, n, lens.data(), images, items, t);
  for (int i = 0; i < n; ++i) free(exact[i]);
}

int main(int argc, char** argv) {
  std::vector<std::vector<unsigned char>> all;
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) fail("cannot open", argv[a], 0, 0);
    std::vector<unsigned char> blob;
    unsigned char buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) blob.insert(blob.end(), buf, buf + got);
    fclose(f);
    all.push_back(blob);
    plan_batch(argv[a], {blob});
    for (size_t cut = 0; cut < blob.size(); ++cut)
      plan_batch(argv[a], {std::vector<unsigned char>(blob.begin(), blob.begin() + cut)});
    // the header ends where the whole file's plan puts the entropy-coded segment
    Image im;
    Item it;
    long long ni = 0;
    parse_one(blob.data(), (long long)blob.size(), 0, &im, &it, 1, &ni);
    const size_t header = im.status == OK ? (size_t)im.scan_off : blob.size();
    for (size_t at = 0; at < header; ++at)
      for (int v = 0; v < 3; ++v) {
        std::vector<unsigned char> alt = blob;
        alt[at] = v == 0 ? 0x00 : v == 1 ? 0xFF : (unsigned char)~blob[at];
        plan_batch(argv[a], {alt});
      }
  }
  all.push_back({});
  all.push_back({0xFF, 0xD8});
  plan_batch("batch", all);
  printf("check_jpeg_plan: %lld plans, %lld images planned OK, all invariants hold\n", g_plans, g_ok);
  return 0;
}
