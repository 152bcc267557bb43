// Robustness of the host JPEG decoder (csrc/host/jpeg.cc) on untrusted bytes,
// as a stand-alone program meant for a sanitizer build (`make asan` builds it
// as build-asan/bin/jpeg_host_test):
//
//   jpeg_host_test <repo>/tests/golden/jpeg
//
// Every *.jpg in the directory is parsed, entropy-decoded and decoded once.
// Then every proper prefix of the restart-marker fixture (f05_*), and 2,000
// seeded single-byte corruptions of it, go through the three calls.  Every
// input buffer is a heap block of exactly the blob's size and every output
// buffer is exactly the size the parse reported, so a read or write past
// either end is an AddressSanitizer report.  Each call must return OK or an
// error code with a message; the program exits 0 when all did.

#include <dirent.h>

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
  long ok = 0, unsupported = 0, malformed = 0, failures = 0;
};

void count(int rc, const char* msg, Tally& t, const char* what) {
  if (rc == TCAMD_JPEG_OK) {
    ++t.ok;
  } else if ((rc == TCAMD_JPEG_UNSUPPORTED || rc == TCAMD_JPEG_MALFORMED) && msg[0]) {
    ++(rc == TCAMD_JPEG_UNSUPPORTED ? t.unsupported : t.malformed);
  } else {
    ++t.failures;
    std::fprintf(stderr, "%s: return code %d with message '%s'\n", what, rc, msg);
  }
}

// the three calls on an exactly-sized copy of the bytes
void exercise(const uint8_t* data, size_t n, Tally& t) {
  std::unique_ptr<uint8_t[]> blob(new uint8_t[n ? n : 1]);
  std::memcpy(blob.get(), data, n);
  char msg[96];
  TcamdJpegInfo info;
  const int rc = tcamd_host_jpeg_parse(blob.get(), n, &info, msg, sizeof(msg));
  count(rc, msg, t, "parse");
  if (rc != TCAMD_JPEG_OK) return;
  if (info.h < 1 || info.w < 1 || info.h > 16384 || info.w > 16384 || (info.ncomp != 1 && info.ncomp != 3)) {
    ++t.failures;
    std::fprintf(stderr, "parse accepted %d x %d x %d\n", info.h, info.w, info.ncomp);
    return;
  }
  if ((uint64_t)info.h * info.w > (64u << 20)) return;  // a corrupted size field: skip the large allocation
  std::unique_ptr<uint8_t[]> coef(new uint8_t[info.coef_bytes]);
  count(tcamd_host_jpeg_entropy_decode(blob.get(), n, coef.get(), info.coef_bytes, msg, sizeof(msg)), msg, t,
        "entropy_decode");
  const uint64_t pixels = (uint64_t)info.h * info.w * info.ncomp;
  std::unique_ptr<uint8_t[]> out(new uint8_t[pixels]);
  count(tcamd_host_jpeg_decode(blob.get(), n, out.get(), pixels, msg, sizeof(msg)), msg, t, "decode");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s <fixture directory>\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1];
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
  Tally whole, prefixes, corrupt;
  std::vector<uint8_t> small;
  for (const std::string& n : names) {
    const std::vector<uint8_t> b = read_file(dir + "/" + n);
    exercise(b.data(), b.size(), whole);
    if (n.compare(0, 4, "f05_") == 0) small = b;
  }
  if (small.empty()) {
    std::fprintf(stderr, "no f05_* fixture under %s\n", dir.c_str());
    return 2;
  }
  for (size_t n = 0; n < small.size(); ++n) exercise(small.data(), n, prefixes);
  uint64_t state = 2000;  // splitmix64
  auto next = [&state]() {
    uint64_t z = (state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  };
  for (int k = 0; k < 2000; ++k) {
    std::vector<uint8_t> m = small;
    m[2 + next() % (m.size() - 2)] = (uint8_t)next();
    exercise(m.data(), m.size(), corrupt);
  }
  const Tally* all[3] = {&whole, &prefixes, &corrupt};
  const char* label[3] = {"fixtures", "prefixes", "corruptions"};
  long failures = 0;
  for (int i = 0; i < 3; ++i) {
    std::printf("%-11s ok %ld, unsupported %ld, malformed %ld, failures %ld\n", label[i], all[i]->ok,
                all[i]->unsupported, all[i]->malformed, all[i]->failures);
    failures += all[i]->failures;
  }
  return failures ? 1 : 0;
}
