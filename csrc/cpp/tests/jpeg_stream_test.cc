// The stream pack and the host emulation of K23 jpeg_huffman
// (csrc/host/jpeg.cc, csrc/kernels/jpeg_huff_core.h) on untrusted bytes, as a
// stand-alone program meant for a sanitizer build (`make asan` builds it as
// build-asan/bin/jpeg_stream_test):
//
//   jpeg_stream_test <repo>/tests/golden/jpeg <repo>/tests/golden/jpeg_huff
//
// Every *.jpg of the directories, f05_* and h05_* with nine variants of what may
// follow a scan in place of their EOI (fill, fill then 00, another scan or DNL
// behind either), every proper prefix of the restart-marker fixture f05_*, and 2,000 seeded single-byte corruptions each of f05_* and of
// the DRI 7 fixture h05_* are packed and, when packable, decoded by the
// emulation, which runs the kernel's own phases and indices.  The blob, the
// stream buffer the emulation reads and the coefficient buffer are heap blocks
// of exactly their size, so a read or write past an end is an AddressSanitizer
// report.  Checked for every input: a blob that does not parse gives the
// parser's code; the emulation's status is 0 exactly when the host entropy
// decoder returns OK, and then the two coefficient buffers are equal.  At
// least 500 corruptions must reach the emulation and at least 50 must end on
// each side, decoded and rejected.  Exits 0 when all held.
//
// Counts with the seeds below (fixtures of this repository):
//   fixtures     inputs 22, not parsed 1, declined 0, decoded 21, rejected 0
//   after scan   inputs 18, not parsed 0, declined 12, decoded 6, rejected 0
//   prefixes     inputs 943, not parsed 629, declined 259, decoded 2, rejected 53
//   corrupt f05  inputs 2000, not parsed 275, declined 26, decoded 1341, rejected 358
//   corrupt h05  inputs 2000, not parsed 14, declined 12, decoded 397, rejected 1577
// The first rejected f05 corruptions are printed: tests/test_jpeg_huffman_gpu.py
// hands three of them (scan bytes 818 = 0x87, 771 = 0x33, 716 = 0x6a) to the GPU.

#include <dirent.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../host/jpeg.cc"

namespace {

std::vector<uint8_t> read_file(const std::string& path) {
  std::vector<uint8_t> v;
  if (FILE* f = std::fopen(path.c_str(), "rb")) {
    uint8_t buf[4096];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
  }
  return v;
}

struct Tally {
  long inputs = 0, not_parsed = 0, declined = 0, decoded = 0, rejected = 0, failures = 0;
};

void fail(Tally& t, const char* what, long a = 0, long b = 0) {
  ++t.failures;
  std::fprintf(stderr, "input %ld: %s (%ld, %ld)\n", t.inputs, what, a, b);
}

void exercise(const uint8_t* data, size_t n, Tally& t) {
  ++t.inputs;
  std::unique_ptr<uint8_t[]> blob(new uint8_t[n ? n : 1]);
  std::memcpy(blob.get(), data, n);
  char msg[96];
  TcamdJpegInfo info, pinfo;
  const int parsed = tcamd_host_jpeg_parse(blob.get(), n, &info, msg, sizeof(msg));
  const uint64_t cap = tcamd_host_jpeg_stream_bound(n);
  std::unique_ptr<uint8_t[]> packed(new uint8_t[cap]);
  uint64_t used = 0;
  const int rc = tcamd_host_jpeg_stream_pack(blob.get(), n, packed.get(), cap, &used, &pinfo, msg, sizeof(msg));
  if (parsed != TCAMD_JPEG_OK) {
    ++t.not_parsed;
    if (rc != parsed) fail(t, "the pack of a blob that does not parse must give the parser's code", rc, parsed);
    return;
  }
  if (rc == TCAMD_JPEG_NOT_PACKABLE) {
    ++t.declined;
    return;
  }
  if (rc != TCAMD_JPEG_OK || used > cap || used < 64 || std::memcmp(&info, &pinfo, sizeof(info)) != 0) {
    fail(t, "pack", rc, (long)used);
    return;
  }
  if ((uint64_t)info.h * info.w > (64u << 20)) return;  // a corrupted size field: skip the large allocation
  std::unique_ptr<uint8_t[]> stream(new uint8_t[used]);
  std::memcpy(stream.get(), packed.get(), used);
  packed.reset();
  std::unique_ptr<uint8_t[]> want(new uint8_t[info.coef_bytes]), got(new uint8_t[info.coef_bytes]);
  std::memset(got.get(), 0x5a, info.coef_bytes);
  const int host = tcamd_host_jpeg_entropy_decode(blob.get(), n, want.get(), info.coef_bytes, msg, sizeof(msg));
  uint32_t status = 99, rounds = 0;
  if (tcamd_host_jpeg_huffman_emulate(stream.get(), got.get(), info.coef_bytes, &status, &rounds) != 0) {
    fail(t, "emulation out of memory");
    return;
  }
  if ((status == 0) != (host == TCAMD_JPEG_OK)) {
    fail(t, "the emulation and the host decoder disagree: status, host code", status, host);
    return;
  }
  if (status == 0) {
    ++t.decoded;
    if (std::memcmp(want.get(), got.get(), info.coef_bytes) != 0) fail(t, "coefficient buffers differ");
  } else {
    ++t.rejected;
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s <fixture directory>...\n", argv[0]);
    return 2;
  }
  Tally whole, after_scan, prefixes, corrupt[2];
  std::vector<uint8_t> picked[2];
  const char* prefix[2] = {"f05_", "h05_"};
  for (int a = 1; a < argc; ++a) {
    const std::string dir = argv[a];
    std::vector<std::string> names;
    if (DIR* d = opendir(dir.c_str())) {
      while (dirent* e = readdir(d)) {
        const std::string n = e->d_name;
        if (n.size() > 4 && n.compare(n.size() - 4, 4, ".jpg") == 0) names.push_back(n);
      }
      closedir(d);
    }
    if (names.empty()) {
      std::fprintf(stderr, "no .jpg under %s\n", dir.c_str());
      return 2;
    }
    std::sort(names.begin(), names.end());
    for (const std::string& n : names) {
      const std::vector<uint8_t> b = read_file(dir + "/" + n);
      exercise(b.data(), b.size(), whole);
      for (int k = 0; k < 2; ++k)
        if (n.compare(0, 4, prefix[k]) == 0) picked[k] = b;
    }
  }
  if (picked[0].empty() || picked[1].empty()) {
    std::fprintf(stderr, "the f05_* and h05_* fixtures are needed\n");
    return 2;
  }
  // what may follow a scan: fill, fill then 00, another scan or DNL behind either
  const std::vector<std::vector<uint8_t>> tails = {
      {}, {0xFF}, {0xFF, 0xFF, 0xFF, 0xD9}, {0xFF, 0xDA, 0x00, 0x02, 0xFF, 0xD9},
      {0xFF, 0xFF, 0x00, 0xFF, 0xDA, 0x00, 0x02, 0xFF, 0xD9}, {0xFF, 0xFF, 0x00, 0xFF, 0xDC, 0x00, 0x04, 0x00, 0x10},
      {0xFF, 0xFF, 0xFF, 0x00, 0x12, 0xFF, 0xD9}, {0xFF, 0xD3, 0xFF, 0xD9}, {0xFF, 0xFF, 0x00}};
  for (int k = 0; k < 2; ++k)
    for (const auto& t : tails) {
      std::vector<uint8_t> m(picked[k].begin(), picked[k].end() - 2);  // without the EOI
      m.insert(m.end(), t.begin(), t.end());
      exercise(m.data(), m.size(), after_scan);
    }
  for (size_t n = 0; n < picked[0].size(); ++n) exercise(picked[0].data(), n, prefixes);
  for (int k = 0; k < 2; ++k) {
    uint64_t state = 2300 + k;  // splitmix64
    auto next = [&state]() {
      uint64_t z = (state += 0x9e3779b97f4a7c15ull);
      z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
      z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
      return z ^ (z >> 31);
    };
    for (int i = 0; i < 2000; ++i) {
      std::vector<uint8_t> m = picked[k];
      const size_t at = 2 + next() % (m.size() - 2);
      const uint8_t v = (uint8_t)next();
      m[at] = v;
      const long before = corrupt[k].rejected;
      exercise(m.data(), m.size(), corrupt[k]);
      // the first few rejected with their markers intact: candidates for the GPU test
      if (k == 0 && corrupt[k].rejected > before && corrupt[k].rejected <= 8)
        std::printf("rejected: f05 byte %zu = 0x%02x\n", at, v);
    }
  }
  const Tally* all[5] = {&whole, &after_scan, &prefixes, &corrupt[0], &corrupt[1]};
  const char* label[5] = {"fixtures", "after scan", "prefixes", "corrupt f05", "corrupt h05"};
  long failures = 0;
  for (int i = 0; i < 5; ++i) {
    std::printf("%-11s inputs %ld, not parsed %ld, declined %ld, decoded %ld, rejected %ld, failures %ld\n", label[i],
                all[i]->inputs, all[i]->not_parsed, all[i]->declined, all[i]->decoded, all[i]->rejected,
                all[i]->failures);
    failures += all[i]->failures;
  }
  for (int k = 0; k < 2; ++k) {
    const long reached = corrupt[k].decoded + corrupt[k].rejected;
    if (reached < 500 || corrupt[k].decoded < 50 || corrupt[k].rejected < 50) {
      std::fprintf(stderr, "%s: too few corruptions reach the emulation or end on one side\n", label[3 + k]);
      ++failures;
    }
  }
  return failures ? 1 : 0;
}
