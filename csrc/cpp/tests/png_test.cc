// The PNG decoder of the host library (csrc/host/png.cc) on untrusted bytes, as
// a stand-alone program meant for a sanitizer build (`make asan` builds it as
// build-asan/bin/png_test):
//
//   png_test <repo>/tests/golden/png
//
// Every *.png of the directory is parsed, inflated into a heap block of exactly
// stage_bytes (when it is not interlaced), unfiltered and decoded into heap
// blocks of exactly pixel_bytes, and the pixels are compared with the .npy next
// to it; the staged route must give the whole decode's pixels.  Then, for the
// two small files named below (a 1-bit grey image and an interlaced 2-bit
// palette image with a short PLTE), every truncation and every single-byte
// corruption (each byte set to each of its 255 other values) goes the same way.
// The blob and every buffer are heap blocks of exactly their size, so a read or
// write past an end is an AddressSanitizer report.  Checked for every input:
// each call returns TCAMD_PNG_OK or an error code with a message; the parse, the
// inflate and the decode agree on whether the headers are good; when both
// routes succeed their pixels are equal.  Exits 0 when all held.
//
// Counts with the fixtures of this repository:
//   fixtures         inputs 12, not parsed 0, parsed but not decoded 0, decoded 12
//   c03 truncations  inputs 140, not parsed 140
//   c03 corruptions  inputs 35700, not parsed 17850, parsed but not decoded 16830, decoded 1020
//   g07 truncations  inputs 95, not parsed 95
//   g07 corruptions  inputs 24225, not parsed 12495, parsed but not decoded 10710, decoded 1020
// (the 1020 are the four CRC bytes of IEND, which the decoder does not check).

#include <dirent.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../host/png.cc"

namespace {

const char* const kSmall[] = {"g07_", "c03_"};

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

// the data of a version 1 .npy file
std::vector<uint8_t> npy_data(const std::vector<uint8_t>& f) {
  if (f.size() < 10 || std::memcmp(f.data(), "\x93NUMPY\x01", 7) != 0) return {};
  const size_t at = 10 + f[8] + 256 * f[9];
  return at <= f.size() ? std::vector<uint8_t>(f.begin() + at, f.end()) : std::vector<uint8_t>();
}

struct Tally {
  long inputs = 0, not_parsed = 0, not_decoded = 0, decoded = 0, failures = 0;
};

void fail(Tally& t, const char* what, long a = 0, long b = 0) {
  ++t.failures;
  std::fprintf(stderr, "input %ld: %s (%ld, %ld)\n", t.inputs, what, a, b);
}

bool code_ok(int rc, const char* msg) {
  return rc == TCAMD_PNG_OK || ((rc == TCAMD_PNG_UNSUPPORTED || rc == TCAMD_PNG_MALFORMED) && msg[0]);
}

// Everything the library does with one blob.  expect: the pixels a good file must give, or null.
void exercise(const uint8_t* data, size_t n, Tally& t, const std::vector<uint8_t>* expect = nullptr) {
  ++t.inputs;
  std::unique_ptr<uint8_t[]> blob(new uint8_t[n ? n : 1]);
  std::memcpy(blob.get(), data, n);
  char msg[96] = "";
  TcamdPngInfo info;
  const int parsed = tcamd_host_png_parse(blob.get(), n, &info, msg, sizeof(msg));
  if (!code_ok(parsed, msg)) fail(t, "parse: code or message", parsed);
  if (parsed != TCAMD_PNG_OK) {
    ++t.not_parsed;
    uint8_t one;
    if (tcamd_host_png_decode(blob.get(), n, &one, 1, msg, sizeof(msg)) != parsed) fail(t, "decode disagrees with parse");
    if (tcamd_host_png_inflate(blob.get(), n, &one, 1, msg, sizeof(msg)) != parsed) fail(t, "inflate disagrees with parse");
    if (expect) fail(t, "a fixture does not parse");
    return;
  }
  if (info.h < 1 || info.w < 1 || info.h > 16384 || info.w > 16384 || info.pixel_bytes > (64u << 20)) {
    ++t.not_decoded;  // a corrupted header that asks for a large image: its size is not what this program explores
    return;
  }
  std::unique_ptr<uint8_t[]> whole(new uint8_t[info.pixel_bytes]);
  const int decoded = tcamd_host_png_decode(blob.get(), n, whole.get(), info.pixel_bytes, msg, sizeof(msg));
  if (!code_ok(decoded, msg)) fail(t, "decode: code or message", decoded);
  if (tcamd_host_png_decode(blob.get(), n, whole.get(), info.pixel_bytes - 1, msg, sizeof(msg)) == TCAMD_PNG_OK)
    fail(t, "decode into a buffer one byte short");
  if (!info.interlace) {
    std::unique_ptr<uint8_t[]> staged(new uint8_t[info.stage_bytes]);
    const int inflated = tcamd_host_png_inflate(blob.get(), n, staged.get(), info.stage_bytes, msg, sizeof(msg));
    if (!code_ok(inflated, msg)) fail(t, "inflate: code or message", inflated);
    if (inflated != decoded) fail(t, "inflate and decode disagree", inflated, decoded);
    if (inflated == TCAMD_PNG_OK) {
      std::unique_ptr<uint8_t[]> pixels(new uint8_t[info.pixel_bytes]);
      if (tcamd_host_png_unfilter(staged.get(), info.stage_bytes, &info, pixels.get(), info.pixel_bytes) != 0)
        fail(t, "unfilter refuses what inflate wrote");
      else if (decoded == TCAMD_PNG_OK && std::memcmp(pixels.get(), whole.get(), info.pixel_bytes) != 0)
        fail(t, "the staged route and the whole decode differ");
      if (tcamd_host_png_unfilter(staged.get(), info.stage_bytes - 1, &info, pixels.get(), info.pixel_bytes) == 0)
        fail(t, "unfilter of staged bytes one byte short");
    }
    if (tcamd_host_png_inflate(blob.get(), n, staged.get(), info.stage_bytes - 1, msg, sizeof(msg)) == TCAMD_PNG_OK)
      fail(t, "inflate into a buffer one byte short");
  }
  if (decoded != TCAMD_PNG_OK) {
    ++t.not_decoded;
    if (expect) fail(t, "a fixture does not decode");
    return;
  }
  ++t.decoded;
  if (expect && (expect->size() != info.pixel_bytes || std::memcmp(expect->data(), whole.get(), info.pixel_bytes) != 0))
    fail(t, "a fixture's pixels are not its .npy", (long)expect->size(), (long)info.pixel_bytes);
}

void report(const char* what, const Tally& t) {
  std::printf("%-12s inputs %ld, not parsed %ld, parsed but not decoded %ld, decoded %ld, failures %ld\n", what, t.inputs,
              t.not_parsed, t.not_decoded, t.decoded, t.failures);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s <fixture directory>...\n", argv[0]);
    return 2;
  }
  long failures = 0;
  int small_seen = 0;
  for (int a = 1; a < argc; ++a) {
    const std::string dir = argv[a];
    std::vector<std::string> names;
    if (DIR* d = opendir(dir.c_str())) {
      while (dirent* e = readdir(d)) {
        const std::string name = e->d_name;
        if (name.size() > 4 && name.compare(name.size() - 4, 4, ".png") == 0) names.push_back(name);
      }
      closedir(d);
    }
    std::sort(names.begin(), names.end());
    Tally fixtures;
    for (const std::string& name : names) {
      const std::vector<uint8_t> blob = read_file(dir + "/" + name);
      const std::vector<uint8_t> want = npy_data(read_file(dir + "/" + name.substr(0, name.size() - 4) + ".npy"));
      if (want.empty()) fail(fixtures, "a fixture without its .npy");
      exercise(blob.data(), blob.size(), fixtures, &want);
    }
    report("fixtures", fixtures);
    if (fixtures.inputs == 0) ++failures;
    failures += fixtures.failures;
    for (const std::string& name : names) {
      if (std::none_of(std::begin(kSmall), std::end(kSmall), [&](const char* p) { return name.rfind(p, 0) == 0; }))
        continue;
      ++small_seen;
      const std::vector<uint8_t> blob = read_file(dir + "/" + name);
      Tally cut, flip;
      for (size_t n = 0; n < blob.size(); ++n) exercise(blob.data(), n, cut);
      std::vector<uint8_t> m = blob;
      for (size_t i = 0; i < blob.size(); ++i) {
        for (int v = 0; v < 256; ++v) {
          if (v == blob[i]) continue;
          m[i] = (uint8_t)v;
          exercise(m.data(), m.size(), flip);
        }
        m[i] = blob[i];
      }
      std::printf("%s (%zu bytes)\n", name.c_str(), blob.size());
      report("truncations", cut);
      report("corruptions", flip);
      if (cut.decoded) fail(cut, "a truncated file decoded");
      failures += cut.failures + flip.failures;
    }
  }
  if (small_seen != 2) {
    std::fprintf(stderr, "expected the two small fixtures, found %d\n", small_seen);
    ++failures;
  }
  std::printf("%s\n", failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
