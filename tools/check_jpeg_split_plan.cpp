// Stand-alone driver of the host split plan (megreader_amd/csrc/jpeg_plan.h: plan_split) for the host sanitizers: no HIP, no
// Python.  The sibling of tools/check_jpeg_plan.cpp, which covers the marker parser itself.
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/check_jpeg_split_plan.cpp \
//       -o check_jpeg_split_plan
//   ./check_jpeg_split_plan tests/golden/jpeg_split/*.jpg tests/golden/jpeg/*.jpg
//
// For every file it plans (a) the file, (b) every prefix of it, (c) the file with each header byte replaced by 0x00, 0xFF and its
// complement, and (d) all files as one batch; each plan is then split with thresholds 0, 1000 and 1 << 20 at 16, 128 and 1024
// bytes.  The split table is an exactly-sized heap block (one entry further is a sanitizer report), and the call is also made
// with one entry too few, which must write nothing.  Every region of every entry must be 16-byte aligned, lie behind the planes
// and inside the grown workspace total, and overlap no other; the program exits non-zero otherwise.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../megreader_amd/csrc/jpeg_plan.h"

using namespace mr::jpeg;

static long long g_plans = 0, g_splits = 0;

static void fail(const char* what, const char* name, long long a, long long b) {
  fprintf(stderr, "FAIL %s: %s (%lld, %lld)\n", name, what, a, b);
  exit(1);
}

static bool same_items(const std::vector<Item>& a, const std::vector<Item>& b, long long n) {
  return n == 0 || memcmp(a.data(), b.data(), sizeof(Item) * (size_t)n) == 0;
}

static void split_one(const char* name, const std::vector<Image>& images, const std::vector<Item>& planned, const Totals& t,
                      long long split_above, int S) {
  const long long n_items = t.n_items;
  std::vector<Item> items(planned.begin(), planned.begin() + n_items);
  long long ws = t.workspace_bytes;
  const long long count = plan_split(images.data(), items.data(), n_items, split_above, S, nullptr, 0, &ws);
  if (count > 0 && (ws != t.workspace_bytes || !same_items(items, planned, n_items)))
    fail("a call without room wrote something", name, count, ws);
  Split* splits = (Split*)malloc(count ? sizeof(Split) * count : 1);   // exactly sized
  if (count > 1) {
    if (plan_split(images.data(), items.data(), n_items, split_above, S, splits, count - 1, &ws) != count ||
        ws != t.workspace_bytes)
      fail("a call with one entry too few wrote something", name, count, ws);
  }
  if (plan_split(images.data(), items.data(), n_items, split_above, S, splits, count, &ws) != count)
    fail("the count changed", name, count, 0);
  ++g_plans;
  g_splits += count;
  if (count == 0 && (ws != t.workspace_bytes || !same_items(items, planned, n_items)))
    fail("a plan without long items changed", name, ws, t.workspace_bytes);
  std::vector<std::pair<long long, long long>> regions;
  long long marked = 0;
  for (long long i = 0; i < n_items; ++i) marked += items[i].reserved != 0;
  if (marked != count) fail("marked items", name, marked, count);
  for (long long k = 0; k < count; ++k) {
    const Split& s = splits[k];
    if (s.item < 0 || s.item >= n_items || items[s.item].reserved != k + 1 || items[s.item].image != s.image)
      fail("item link", name, k, s.item);
    const Item& it = items[s.item];
    const Image& im = images[s.image];
    if (im.status != OK || it.len <= split_above) fail("a short item was split", name, it.len, split_above);
    if (s.subseq_bytes != S || s.n_sub != (it.len + S - 1) / S || s.n_wg != (s.n_sub + SPLIT_WG - 1) / SPLIT_WG || s.n_sub < 1)
      fail("sub-sequence counts", name, s.n_sub, s.n_wg);
    if (s.blocks_per_mcu != (im.ncomp == 3 ? im.hs * im.vs + 2 : 1) || s.n_blocks != it.nmcu * s.blocks_per_mcu || s.n_blocks < 1)
      fail("block counts", name, s.n_blocks, s.blocks_per_mcu);
    if (s.raw_bytes < (long long)s.n_sub * S + 16 || s.raw_bytes < it.len + 16) fail("raw bytes", name, s.raw_bytes, it.len);
    if (s.coef_bytes != align16(4LL * s.n_blocks) + 128LL * s.n_blocks) fail("coefficient bytes", name, s.coef_bytes, s.n_blocks);
    const std::pair<long long, long long> mine[] = {{s.meta_off, 16},           {s.raw_off, s.raw_bytes},
                                                    {s.in_off, 8LL * s.n_sub},  {s.exit_off, 8LL * s.n_sub},
                                                    {s.wg_exit_off, 16LL * s.n_wg}, {s.block_off, 4LL * s.n_sub},
                                                    {s.coef_off, s.coef_bytes}};
    for (const auto& r : mine) {
      if (r.first % 16 || r.first < t.workspace_bytes || r.second <= 0 || r.first + r.second > ws)
        fail("region outside the workspace", name, r.first, r.second);
      regions.push_back(r);
    }
  }
  std::sort(regions.begin(), regions.end());
  for (size_t i = 1; i < regions.size(); ++i)
    if (regions[i - 1].first + regions[i - 1].second > regions[i].first) fail("regions overlap", name, regions[i].first, 0);
  free(splits);
}

static void plan_batch(const char* name, const std::vector<std::vector<unsigned char>>& blobs) {
  const int n = (int)blobs.size();
  std::vector<unsigned char*> exact(n);
  std::vector<const void*> ptrs(n);
  std::vector<long long> lens(n);
  for (int i = 0; i < n; ++i) {
    lens[i] = (long long)blobs[i].size();
    exact[i] = (unsigned char*)malloc(blobs[i].size() ? blobs[i].size() : 1);
    if (!blobs[i].empty()) memcpy(exact[i], blobs[i].data(), blobs[i].size());
    ptrs[i] = blobs[i].empty() ? nullptr : exact[i];
  }
  std::vector<Image> images(n);
  std::vector<Item> items(4);
  Totals t;
  plan(n, ptrs.data(), lens.data(), images.data(), items.data(), (long long)items.size(), &t);
  if (t.n_items > (long long)items.size()) {
    items.resize((size_t)t.n_items);
    plan(n, ptrs.data(), lens.data(), images.data(), items.data(), (long long)items.size(), &t);
  }
  const long long above[] = {0, 1000, 1LL << 20};
  const int sizes[] = {16, 128, 1024};
  for (long long a : above)
    for (int S : sizes) split_one(name, images, items, t, a, S);
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
  printf("check_jpeg_split_plan: %lld split plans, %lld split items, all invariants hold\n", g_plans, g_splits);
  return 0;
}
