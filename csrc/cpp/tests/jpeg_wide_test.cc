// The wide stream pack and the host emulation of the K24 jpeg_huffman_wide
// launch sequence (csrc/host/jpeg.cc, csrc/kernels/jpeg_huff_wide_core.h) on
// untrusted bytes, as a stand-alone program meant for a sanitizer build
// (`make asan` builds it as build-asan/bin/jpeg_wide_test):
//
//   jpeg_wide_test <repo>/tests/golden/jpeg <repo>/tests/golden/jpeg_huff <repo>/tests/golden/jpeg_wide
//
// Every *.jpg of the directories, every proper prefix of the restart-marker
// fixture f05_* and 2,000 seeded single-byte corruptions each of f05_* and of
// the DRI 7 fixture h05_* (the seeds of jpeg_stream_test.cc) are packed at
// scales 1 and 2 and, when packable, decoded by the emulation in chunks of 2
// and of 1024 subsequences.  The emulation runs the kernels' own phases and
// indices; the blob, the stream buffer, the coefficient buffer and (inside the
// emulation) the workspace are heap blocks of exactly their size, so a read or
// write past an end is an AddressSanitizer report.  Checked for every input,
// scale and chunk size: a blob that does not parse gives the parser's code;
// the emulation's status is 0 exactly when the host entropy decoder returns OK
// at that scale, and then the two coefficient buffers are equal.  At least 500
// corruptions must reach the emulation and at least 50 must end on each side,
// decoded and rejected.  Exits 0 when all held.
//
// Counts with the seeds below (fixtures of this repository), the same at both
// scales and both chunk sizes, and those of jpeg_stream_test.cc plus w01:
//   fixtures     inputs 23, not parsed 1, declined 0, decoded 22, rejected 0
//   prefixes     inputs 943, not parsed 629, declined 259, decoded 2, rejected 53
//   corrupt f05  inputs 2000, not parsed 275, declined 26, decoded 1341, rejected 358
//   corrupt h05  inputs 2000, not parsed 14, declined 12, decoded 397, rejected 1577

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

void exercise(const uint8_t* data, size_t n, int scale, uint32_t chunk_subs, Tally& t) {
  ++t.inputs;
  std::unique_ptr<uint8_t[]> blob(new uint8_t[n ? n : 1]);
  std::memcpy(blob.get(), data, n);
  char msg[96];
  TcamdJpegInfo info, pinfo;
  const int parsed = tcamd_host_jpeg_parse_scaled(blob.get(), n, scale, &info, msg, sizeof(msg));
  const uint64_t cap = tcamd_host_jpeg_stream_bound_wide(n);
  std::unique_ptr<uint8_t[]> packed(new uint8_t[cap]);
  uint64_t used = 0;
  uint32_t nsub = 0;
  const int rc = tcamd_host_jpeg_stream_pack_wide(blob.get(), n, scale, packed.get(), cap, &used, &nsub, &pinfo, msg,
                                                  sizeof(msg));
  if (parsed != TCAMD_JPEG_OK) {
    ++t.not_parsed;
    if (rc != parsed) fail(t, "the pack of a blob that does not parse must give the parser's code", rc, parsed);
    return;
  }
  if (rc == TCAMD_JPEG_NOT_PACKABLE) {
    ++t.declined;
    return;
  }
  if (rc != TCAMD_JPEG_OK || used > cap || used < 64 || nsub == 0 || std::memcmp(&info, &pinfo, sizeof(info)) != 0) {
    fail(t, "pack", rc, (long)used);
    return;
  }
  if ((uint64_t)info.h * info.w * scale * scale > (64u << 20)) return;  // a corrupted size field: skip the large allocation
  std::unique_ptr<uint8_t[]> stream(new uint8_t[used]);
  std::memcpy(stream.get(), packed.get(), used);
  packed.reset();
  std::unique_ptr<uint8_t[]> want(new uint8_t[info.coef_bytes]), got(new uint8_t[info.coef_bytes]);
  std::memset(got.get(), 0x5a, info.coef_bytes);
  const int host =
      tcamd_host_jpeg_entropy_decode_scaled(blob.get(), n, scale, want.get(), info.coef_bytes, msg, sizeof(msg));
  uint32_t status = 99, changed = 0;
  if (tcamd_host_jpeg_huffman_wide_emulate(stream.get(), got.get(), info.coef_bytes, chunk_subs, &status, &changed) !=
      0) {
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
  const int scales[2] = {1, 2};
  const uint32_t chunks[2] = {2, 1024};
  long failures = 0;
  std::vector<std::vector<uint8_t>> blobs;
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
      blobs.push_back(read_file(dir + "/" + n));
      for (int k = 0; k < 2; ++k)
        if (n.compare(0, 4, prefix[k]) == 0) picked[k] = blobs.back();
    }
  }
  if (picked[0].empty() || picked[1].empty()) {
    std::fprintf(stderr, "the f05_* and h05_* fixtures are needed\n");
    return 2;
  }
  for (int si = 0; si < 2; ++si) {
    for (int ci = 0; ci < 2; ++ci) {
      const int scale = scales[si];
      const uint32_t cs = chunks[ci];
      Tally whole, prefixes, corrupt[2];
      for (const auto& b : blobs) exercise(b.data(), b.size(), scale, cs, whole);
      for (size_t n = 0; n < picked[0].size(); ++n) exercise(picked[0].data(), n, scale, cs, prefixes);
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
          m[at] = (uint8_t)next();
          exercise(m.data(), m.size(), scale, cs, corrupt[k]);
        }
      }
      const Tally* all[4] = {&whole, &prefixes, &corrupt[0], &corrupt[1]};
      const char* label[4] = {"fixtures", "prefixes", "corrupt f05", "corrupt h05"};
      std::printf("scale %d, chunks of %u\n", scale, cs);
      for (int i = 0; i < 4; ++i) {
        std::printf("  %-11s inputs %ld, not parsed %ld, declined %ld, decoded %ld, rejected %ld, failures %ld\n", label[i],
                    all[i]->inputs, all[i]->not_parsed, all[i]->declined, all[i]->decoded, all[i]->rejected,
                    all[i]->failures);
        failures += all[i]->failures;
      }
      for (int k = 0; k < 2; ++k) {
        const long reached = corrupt[k].decoded + corrupt[k].rejected;
        if (reached < 500 || corrupt[k].decoded < 50 || corrupt[k].rejected < 50) {
          std::fprintf(stderr, "%s: too few corruptions reach the emulation or end on one side\n", label[2 + k]);
          ++failures;
        }
      }
    }
  }
  return failures ? 1 : 0;
}
