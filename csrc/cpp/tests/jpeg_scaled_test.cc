// The reduced-size JPEG decode of the host (csrc/host/jpeg.cc: scaled parse,
// entropy decode into the compact coefficient buffer, decode to pixels) on
// untrusted bytes, as a stand-alone program meant for a sanitizer build (`make
// asan` builds it as build-asan/bin/jpeg_scaled_test):
//
//   jpeg_scaled_test <repo>/tests/golden/jpeg
//
// Every *.jpg of the directory, every proper prefix of f05_* (4:2:0 with restart
// markers) and f03_* (4:2:2), and 500 seeded single-byte corruptions of f05_*
// per scale go through the three scaled entry points at scales 1, 2, 4 and 8.
// The blob, the coefficient buffer and the pixel buffer are heap blocks of
// exactly their capacity between 32 guard bytes each, so a write past an end is
// an AddressSanitizer report, and without a sanitizer a changed guard byte.
// Checked for every input and scale:
//   - the three calls return the code and the message of the full-size calls;
//   - at scale 1 info, coefficients and pixels equal those of the full-size
//     entry points byte for byte;
//   - at scales 2, 4, 8 the shape is ceil(H / s) x ceil(W / s), coef_off is
//     16-byte aligned, every stored coefficient equals the one at its
//     frequency in the full-size buffer, and the pixels equal the
//     reconstruction of the compact buffer;
//   - a capacity one byte short is "coefficient buffer too small" / "pixel
//     buffer too small" and writes nothing.
// Exits 0 when all held.
//
// Counts with the seeds below (fixtures of this repository), at every scale:
//   fixtures   inputs 17, decoded 16, refused 1
//   prefixes   inputs 2174, decoded 4, refused 2170
//   corrupt    inputs 500, decoded 331 to 350, refused 150 to 169 (the seed follows the scale)

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

constexpr size_t kGuard = 32;
constexpr uint8_t kGuardByte = 0xC7;

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

// n bytes between guards, 16-byte aligned like the buffers of the callers
struct Guarded {
  std::unique_ptr<uint8_t[]> store;
  size_t n;
  explicit Guarded(size_t n_) : store(new uint8_t[n_ + 2 * kGuard + 16]), n(n_) {
    std::memset(store.get(), kGuardByte, n + 2 * kGuard + 16);
  }
  uint8_t* data() const {
    uint8_t* p = store.get() + kGuard;
    return p + (16 - reinterpret_cast<uintptr_t>(p) % 16) % 16;
  }
  bool intact(bool untouched = false) const {
    const uint8_t* d = data();
    for (const uint8_t* p = store.get(); p < d; ++p)
      if (*p != kGuardByte) return false;
    for (const uint8_t* p = d + n; p < store.get() + n + 2 * kGuard + 16; ++p)
      if (*p != kGuardByte) return false;
    if (untouched)
      for (size_t i = 0; i < n; ++i)
        if (d[i] != kGuardByte) return false;
    return true;
  }
};

struct Tally {
  long inputs = 0, decoded = 0, refused = 0, failures = 0;
};

void fail(Tally& t, int scale, const char* what, long a = 0, long b = 0) {
  ++t.failures;
  std::fprintf(stderr, "input %ld at 1/%d: %s (%ld, %ld)\n", t.inputs, scale, what, a, b);
}

void exercise(const uint8_t* data, size_t n, int scale, Tally& t) {
  ++t.inputs;
  std::unique_ptr<uint8_t[]> blob(new uint8_t[n ? n : 1]);
  std::memcpy(blob.get(), data, n);
  char msg[96], fmsg[96];
  TcamdJpegInfo full, info;
  const int fparsed = tcamd_host_jpeg_parse(blob.get(), n, &full, fmsg, sizeof(fmsg));
  const int parsed = tcamd_host_jpeg_parse_scaled(blob.get(), n, scale, &info, msg, sizeof(msg));
  if (parsed != fparsed || std::strcmp(msg, fmsg) != 0) return fail(t, scale, "parse: code or message", parsed, fparsed);
  if (parsed != TCAMD_JPEG_OK) {
    ++t.refused;
    uint8_t dummy[16];
    if (tcamd_host_jpeg_decode_scaled(blob.get(), n, scale, dummy, 0, msg, sizeof(msg)) != parsed ||
        std::strcmp(msg, fmsg) != 0)
      fail(t, scale, "decode of a blob that does not parse");
    return;
  }
  if ((uint64_t)full.h * full.w > (64u << 20)) return;  // a corrupted size field: skip the large allocation
  if (info.h != (full.h + scale - 1) / scale || info.w != (full.w + scale - 1) / scale || info.scale != scale ||
      info.ncomp != full.ncomp)
    return fail(t, scale, "shape", info.h, info.w);
  uint64_t end = (uint64_t)info.ncomp * 128;
  for (int c = 0; c < info.ncomp; ++c) {
    if (info.coef_off[c] % 16 || info.coef_off[c] < end || info.coef_off[c] >= end + 16 || info.bw[c] != full.bw[c] ||
        info.bh[c] != full.bh[c])
      return fail(t, scale, "layout", c, (long)info.coef_off[c]);
    end = info.coef_off[c] + (uint64_t)info.bw[c] * info.bh[c] * info.ny[c] * info.nx[c] * 2;
  }
  if (end != info.coef_bytes) return fail(t, scale, "coef_bytes", (long)end, (long)info.coef_bytes);
  if (scale == 1 && std::memcmp(&info, &full, sizeof(info)) != 0) return fail(t, scale, "the parse at scale 1");

  const uint64_t pixel_bytes = (uint64_t)info.h * info.w * info.ncomp;
  Guarded fcoef(full.coef_bytes), coef(info.coef_bytes), shortc(info.coef_bytes - 1);
  Guarded fpix((uint64_t)full.h * full.w * full.ncomp), pix(pixel_bytes), shortp(pixel_bytes - 1);
  const int fe = tcamd_host_jpeg_entropy_decode(blob.get(), n, fcoef.data(), fcoef.n, fmsg, sizeof(fmsg));
  const int e = tcamd_host_jpeg_entropy_decode_scaled(blob.get(), n, scale, coef.data(), coef.n, msg, sizeof(msg));
  if (e != fe || std::strcmp(msg, fmsg) != 0) fail(t, scale, "entropy decode: code or message", e, fe);
  const int fd = tcamd_host_jpeg_decode(blob.get(), n, fpix.data(), fpix.n, fmsg, sizeof(fmsg));
  const int d = tcamd_host_jpeg_decode_scaled(blob.get(), n, scale, pix.data(), pix.n, msg, sizeof(msg));
  if (d != fd || std::strcmp(msg, fmsg) != 0) fail(t, scale, "decode: code or message", d, fd);
  if (d != e) fail(t, scale, "decode and entropy decode disagree", d, e);
  if (tcamd_host_jpeg_entropy_decode_scaled(blob.get(), n, scale, shortc.data(), shortc.n, msg, sizeof(msg)) !=
          TCAMD_JPEG_MALFORMED ||
      std::strcmp(msg, "coefficient buffer too small") != 0 || !shortc.intact(true))
    fail(t, scale, "a coefficient buffer one byte short");
  if (tcamd_host_jpeg_decode_scaled(blob.get(), n, scale, shortp.data(), shortp.n, msg, sizeof(msg)) !=
          TCAMD_JPEG_MALFORMED ||
      std::strcmp(msg, "pixel buffer too small") != 0 || !shortp.intact(true))
    fail(t, scale, "a pixel buffer one byte short");
  if (!fcoef.intact() || !coef.intact() || !fpix.intact() || !pix.intact()) fail(t, scale, "a guard byte was written");
  if (e != TCAMD_JPEG_OK) {
    ++t.refused;
    return;
  }
  ++t.decoded;
  if (scale == 1) {
    if (std::memcmp(coef.data(), fcoef.data(), coef.n) != 0) fail(t, scale, "coefficients at scale 1");
    if (std::memcmp(pix.data(), fpix.data(), pix.n) != 0) fail(t, scale, "pixels at scale 1");
    return;
  }
  if (std::memcmp(coef.data(), fcoef.data(), (size_t)info.ncomp * 128) != 0) fail(t, scale, "quantisation tables");
  for (int c = 0; c < info.ncomp; ++c) {
    const int16_t* a = reinterpret_cast<const int16_t*>(coef.data() + info.coef_off[c]);
    const int16_t* b = reinterpret_cast<const int16_t*>(fcoef.data() + full.coef_off[c]);
    const int ny = info.ny[c], nx = info.nx[c];
    for (int64_t k = 0; k < (int64_t)info.bw[c] * info.bh[c]; ++k)
      for (int v = 0; v < ny; ++v)
        for (int u = 0; u < nx; ++u)
          if (a[k * ny * nx + v * nx + u] != b[k * 64 + v * 8 + u]) return fail(t, scale, "a stored coefficient", c, (long)k);
  }
  Guarded again(pixel_bytes);
  reconstruct_scaled(info, coef.data(), again.data());
  if (!again.intact() || std::memcmp(again.data(), pix.data(), pix.n) != 0)
    fail(t, scale, "pixels against the reconstruction of the compact buffer");
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
  std::sort(names.begin(), names.end());
  std::vector<uint8_t> f05, f03;
  std::vector<std::vector<uint8_t>> blobs;
  for (const std::string& n : names) {
    blobs.push_back(read_file(dir + "/" + n));
    if (n.compare(0, 4, "f05_") == 0) f05 = blobs.back();
    if (n.compare(0, 4, "f03_") == 0) f03 = blobs.back();
  }
  if (f05.empty() || f03.empty()) {
    std::fprintf(stderr, "the f03_* and f05_* fixtures are needed under %s\n", dir.c_str());
    return 2;
  }
  long failures = 0;
  const int scales[4] = {1, 2, 4, 8};
  for (int scale : scales) {
    Tally whole, prefixes, corrupt;
    for (const auto& b : blobs) exercise(b.data(), b.size(), scale, whole);
    for (const auto* b : {&f05, &f03})
      for (size_t n = 0; n < b->size(); ++n) exercise(b->data(), n, scale, prefixes);
    uint64_t state = 2400 + scale;  // splitmix64
    auto next = [&state]() {
      uint64_t z = (state += 0x9e3779b97f4a7c15ull);
      z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
      z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
      return z ^ (z >> 31);
    };
    for (int i = 0; i < 500; ++i) {
      std::vector<uint8_t> m = f05;
      m[2 + next() % (m.size() - 2)] = (uint8_t)next();
      exercise(m.data(), m.size(), scale, corrupt);
    }
    const Tally* all[3] = {&whole, &prefixes, &corrupt};
    const char* label[3] = {"fixtures", "prefixes", "corrupt"};
    for (int i = 0; i < 3; ++i) {
      std::printf("1/%d %-9s inputs %ld, decoded %ld, refused %ld, failures %ld\n", scale, label[i], all[i]->inputs,
                  all[i]->decoded, all[i]->refused, all[i]->failures);
      failures += all[i]->failures;
    }
    if (whole.decoded < 10 || corrupt.decoded < 50 || corrupt.refused < 50) {
      std::fprintf(stderr, "1/%d: too few inputs decoded or refused\n", scale);
      ++failures;
    }
  }
  return failures ? 1 : 0;
}
