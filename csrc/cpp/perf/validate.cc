// perf_analyzer Validator: every response's outputs against the expectation of
// the data entry its request carried ("validation_data" of the --input-data
// JSON, or the entry's first response with --validate-outputs first), by the
// rule of kernels/compare_math.h.
//
// In-band results and system shared memory are compared here, on the thread the
// response completes on.  Outputs in HIP shared memory never leave the device:
// one K26 launch (tcamd_compare_expected of libtcamd_hip.so) per response on the
// lane's stream compares all its outputs, one small async copy takes the records
// to a pinned ring, and the profiler reads the ring once per window.  A slot
// alternates between two sets of output regions and owns one event, recorded
// after each of its compares: before a compare is queued the slot waits for the
// one before it, which was queued a whole request earlier, so the set the next
// request but one writes to is no longer being read.  (The open-loop rate mode
// hands a slot its next request whether or not the last one has answered, as it
// always did; output regions are only private to a request while no more than
// the prepared 64 slots are in flight.)
#include <cinttypes>
#include <cstring>

#include <hip/hip_runtime_api.h>

#include "../../kernels/compare_math.h"
#include "perf.h"

namespace tcperf {

namespace {

typedef int (*CompareFn)(const TcamdComparePair*, int, double, double, TcamdCompareRecord*, void*);

constexpr size_t kRing = 1 << 14;  // responses between two read-backs before a compare has to wait for one

// dtype codes of csrc/kernels/common.h; BYTES is compared as UINT8 over its serialized bytes
int CompareDtype(const std::string& dt)
{
  static const std::map<std::string, int> m = {
      {"BOOL", 0}, {"INT8", 1}, {"INT16", 2}, {"INT32", 3}, {"INT64", 4}, {"UINT8", 5}, {"UINT16", 6},
      {"UINT32", 7}, {"UINT64", 8}, {"FP16", 9}, {"FP32", 10}, {"FP64", 11}, {"BF16", 12}, {"BYTES", 5}};
  auto it = m.find(dt);
  return it == m.end() ? -1 : it->second;
}

std::string FormatBits(const std::string& dt, uint64_t bits)
{
  char b[64];
  if (dt == "FP32") {
    snprintf(b, sizeof(b), "%.9g", static_cast<double>(tcamd_cmp::f32_of(static_cast<uint32_t>(bits))));
  } else if (dt == "FP64") {
    snprintf(b, sizeof(b), "%.17g", tcamd_cmp::f64_of(bits));
  } else if (dt == "FP16") {
    const uint32_t wide = tcamd_cmp::f16_to_f32_bits(static_cast<uint32_t>(bits));
    snprintf(b, sizeof(b), "%.6g", static_cast<double>(tcamd_cmp::f32_of(wide)));
  } else if (dt == "BF16") {
    snprintf(b, sizeof(b), "%.6g", static_cast<double>(tcamd_cmp::f32_of(static_cast<uint32_t>(bits) << 16)));
  } else if (dt == "INT8") {
    snprintf(b, sizeof(b), "%d", static_cast<int>(static_cast<int8_t>(bits)));
  } else if (dt == "INT16") {
    snprintf(b, sizeof(b), "%d", static_cast<int>(static_cast<int16_t>(bits)));
  } else if (dt == "INT32") {
    snprintf(b, sizeof(b), "%d", static_cast<int>(static_cast<int32_t>(bits)));
  } else if (dt == "INT64") {
    snprintf(b, sizeof(b), "%" PRId64, static_cast<int64_t>(bits));
  } else if (dt == "BYTES") {
    snprintf(b, sizeof(b), "0x%02x", static_cast<unsigned>(bits));
  } else {
    snprintf(b, sizeof(b), "%" PRIu64, bits);
  }
  return b;
}

std::string FailureLine(const TensorSpec& t, size_t entry, const TcamdCompareRecord& r)
{
  char b[256];
  snprintf(b, sizeof(b), "output %s of data entry %zu: element %" PRIu64 " is %s, expected %s (%" PRIu64
           " mismatching element(s), largest difference %g)",
           t.name.c_str(), entry, r.first_index, FormatBits(t.datatype, r.got_bits).c_str(),
           FormatBits(t.datatype, r.expected_bits).c_str(), r.mismatches, r.max_abs_diff);
  return b;
}

std::string SizeLine(const TensorSpec& t, size_t entry, size_t got, size_t want)
{
  return "output " + t.name + " of data entry " + std::to_string(entry) + ": the response holds " +
         std::to_string(got) + " bytes, the expectation " + std::to_string(want);
}

}  // namespace

struct Validator::Pending {
  size_t entry = 0;
  int n = 0;                              // pairs of the launch
  int output[tcamd_cmp::kMaxPairs] = {};  // pair -> output index
};

Validator::Validator(const Options& o, DataSet* data, size_t slots) : o_(o), data_(data)
{
  const auto& specs = data_->OutputSpecs();
  if (specs.size() > static_cast<size_t>(tcamd_cmp::kMaxPairs)) {
    setup_error_ = "output validation takes at most 64 outputs per response";
    return;
  }
  for (const auto& t : specs)
    if (CompareDtype(t.datatype) < 0) {
      setup_error_ = "output validation: unsupported datatype " + t.datatype + " of " + t.name;
      return;
    }
  if (!tcamd_cmp::tol_valid(o.validation_atol, o.validation_rtol)) {
    setup_error_ = "--validation-tolerance must be finite and not negative";
    return;
  }
  if (!data_->DeviceOutputs()) return;
  compare_fn_ = HipKernelSymbol("tcamd_compare_expected");
  if (!compare_fn_) {
    setup_error_ = "validating HIP shm outputs needs K26 (tcamd_compare_expected in libtcamd_hip.so)";
    return;
  }
  hipError_t he = hipSetDevice(data_->Device());
  const size_t bytes = kRing * specs.size() * sizeof(TcamdCompareRecord);
  if (he == hipSuccess) he = hipMalloc(&dev_records_, bytes);
  if (he == hipSuccess) he = hipHostMalloc(&host_records_, bytes, hipHostMallocDefault);
  events_.assign(slots, nullptr);
  event_set_.assign(slots, false);
  for (size_t i = 0; i < slots && he == hipSuccess; ++i) {
    hipEvent_t ev;
    he = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    events_[i] = ev;
  }
  if (he != hipSuccess) setup_error_ = std::string("validator setup failed: ") + hipGetErrorString(he);
  ring_.resize(kRing);
}

Validator::~Validator()
{
  if (!data_->DeviceOutputs()) return;
  (void)hipSetDevice(data_->Device());
  if (data_->Stream()) (void)hipStreamSynchronize(static_cast<hipStream_t>(data_->Stream()));
  for (void* ev : events_)
    if (ev) (void)hipEventDestroy(static_cast<hipEvent_t>(ev));
  if (dev_records_) (void)hipFree(dev_records_);
  if (host_records_) (void)hipHostFree(host_records_);
}

void Validator::Fail(const std::string& line)
{
  ++failed_;
  if (first_failure_.empty()) first_failure_ = line;
}

std::string Validator::FirstFailure()
{
  std::lock_guard<std::mutex> lk(mu_);
  return first_failure_;
}

void Validator::Check(size_t slot, int set, size_t entry, const InferResult* r)
{
  const auto& specs = data_->OutputSpecs();
  const bool shm = data_->SharedOutputs(), dev = data_->DeviceOutputs(), first = data_->ValidateFirst();
  const tcamd_cmp::Tol tol = tcamd_cmp::make_tol(o_.validation_atol, o_.validation_rtol);
  hipStream_t st = static_cast<hipStream_t>(data_->Stream());
  std::unique_lock<std::mutex> lk(mu_, std::defer_lock);
  if (dev) {
    // HIP calls of this thread go to the lane's GPU; the slot's previous
    // compare (queued a request ago) has normally retired already
    (void)hipSetDevice(data_->Device());
    if (slot < events_.size() && event_set_[slot]) (void)hipEventSynchronize(static_cast<hipEvent_t>(events_[slot]));
    lk.lock();
    if (head_ - tail_ >= kRing) Drain();
  }
  TcamdComparePair pairs[tcamd_cmp::kMaxPairs];
  Pending pend;
  pend.entry = entry;
  bool counted = false, failed = false;
  double host_max = 0;
  std::string line;
  for (size_t oi = 0; oi < specs.size(); ++oi) {
    const TensorSpec& t = specs[oi];
    if (!lk.owns_lock()) lk.lock();  // expectations of "first" are written under the lock
    DataSet::Expectation& x = data_->Expect(entry, oi);
    if (!x.named) {
      if (!dev) lk.unlock();
      continue;
    }
    // where the output is and, where known, how large
    const uint8_t* got = nullptr;
    size_t got_size = 0, cap = 0;
    bool size_known = false;
    if (!shm) {
      if (!r || !r->RawData(t.name, &got, &got_size).IsOk()) {
        Fail("output " + t.name + " of data entry " + std::to_string(entry) + ": missing from the response");
        failed = counted = true;
        if (!dev) lk.unlock();
        continue;
      }
      size_known = true;
    } else {
      got = static_cast<const uint8_t*>(data_->OutputPtr(slot, set, oi, &cap));
      std::vector<int64_t> shape;
      const size_t es = static_cast<size_t>(tcamd_cmp::kind_width(tcamd_cmp::kind_of(CompareDtype(t.datatype))));
      if (t.datatype != "BYTES" && r && r->Shape(t.name, &shape).IsOk() && !shape.empty()) {
        got_size = es;
        for (auto d : shape) got_size *= static_cast<size_t>(d < 0 ? 0 : d);
        size_known = true;
      }
    }
    if (first && !x.have) {
      // the first response of this entry becomes its expectation
      x.size = size_known ? got_size : cap;
      if (x.size > cap && shm) x.size = cap;
      if (dev) {
        hipError_t he = hipMalloc(&x.dev, std::max<size_t>(x.size, 16));
        if (he == hipSuccess) he = hipMemcpyAsync(x.dev, got, x.size, hipMemcpyDeviceToDevice, st);
        if (he != hipSuccess) {
          Fail(std::string("capturing the expectation failed: ") + hipGetErrorString(he));
          failed = counted = true;
          continue;
        }
      } else {
        x.bytes.assign(got, got + x.size);
      }
      x.have = true;
      if (!dev) lk.unlock();
      continue;
    }
    const size_t want = x.size;
    if (!dev) lk.unlock();  // a filled expectation does not change any more
    counted = true;
    if ((size_known && got_size != want) || (shm && want > cap)) {
      if (line.empty()) line = SizeLine(t, entry, size_known ? got_size : cap, want);
      failed = true;
      continue;
    }
    const int dt = CompareDtype(t.datatype);
    const uint64_t count = want / static_cast<size_t>(tcamd_cmp::kind_width(tcamd_cmp::kind_of(dt)));
    if (dev) {
      pend.output[pend.n] = static_cast<int>(oi);
      pairs[pend.n++] = {got, x.dev, count, dt, 0};
      continue;
    }
    TcamdCompareRecord rec;
    const TcamdComparePair p = {got, x.bytes.data(), count, dt, 0};
    tcamd_cmp::compare_host(p, tol, &rec);
    if (rec.max_abs_diff > host_max) host_max = rec.max_abs_diff;
    if (rec.mismatches) {
      if (line.empty()) line = FailureLine(t, entry, rec);
      failed = true;
    }
  }
  if (dev) {
    // one launch for the response, its records into the ring, then the slot's event
    if (failed) pend.n = 0;  // already counted as failed: nothing more to learn from a launch
    if (pend.n) {
      const size_t at = (head_ % kRing) * specs.size() * sizeof(TcamdCompareRecord);
      auto* drec = reinterpret_cast<TcamdCompareRecord*>(static_cast<uint8_t*>(dev_records_) + at);
      const auto k26 = reinterpret_cast<CompareFn>(compare_fn_);
      int rc = k26(pairs, pend.n, o_.validation_atol, o_.validation_rtol, drec, st);
      if (rc == 0)
        rc = hipMemcpyAsync(static_cast<uint8_t*>(host_records_) + at, drec, pend.n * sizeof(TcamdCompareRecord),
                            hipMemcpyDeviceToHost, st);
      if (rc != 0) {
        if (line.empty())
          line = "K26 compare_expected failed: " + std::string(hipGetErrorString(static_cast<hipError_t>(rc)));
        failed = true;
      } else {
        ring_[head_ % kRing] = pend;
        ++head_;
        counted = false;  // counted when its records are read
      }
    }
    if (slot < events_.size() && hipEventRecord(static_cast<hipEvent_t>(events_[slot]), st) == hipSuccess)
      event_set_[slot] = true;
  }
  if (!lk.owns_lock()) lk.lock();
  if (host_max > max_diff_) max_diff_ = host_max;
  if (failed) {
    if (!line.empty()) Fail(line);
  } else if (counted) {
    ++validated_;
  }
}

// mu_ held: wait for the lane's stream, then read the records of every queued launch
void Validator::Drain()
{
  if (head_ == tail_) return;
  (void)hipSetDevice(data_->Device());
  const hipError_t he = hipStreamSynchronize(static_cast<hipStream_t>(data_->Stream()));
  const auto& specs = data_->OutputSpecs();
  for (; tail_ != head_; ++tail_) {
    if (he != hipSuccess) {
      Fail(std::string("reading the compare records failed: ") + hipGetErrorString(he));
      continue;
    }
    const Pending& p = ring_[tail_ % kRing];
    const size_t at = (tail_ % kRing) * specs.size() * sizeof(TcamdCompareRecord);
    const auto* rec = reinterpret_cast<const TcamdCompareRecord*>(static_cast<const uint8_t*>(host_records_) + at);
    bool bad = false;
    for (int i = 0; i < p.n; ++i) {
      if (rec[i].max_abs_diff > max_diff_) max_diff_ = rec[i].max_abs_diff;
      if (rec[i].mismatches) {
        if (!bad) Fail(FailureLine(specs[p.output[i]], p.entry, rec[i]));
        bad = true;
      }
    }
    if (!bad) ++validated_;
  }
}

void Validator::Collect(uint64_t* validated, uint64_t* failed, double* max_abs_diff)
{
  std::lock_guard<std::mutex> lk(mu_);
  if (data_->DeviceOutputs()) Drain();
  *validated = validated_;
  *failed = failed_;
  validated_total_ += validated_;
  failed_total_ += failed_;
  if (max_abs_diff) *max_abs_diff = max_diff_;
  validated_ = failed_ = 0;
  max_diff_ = 0;
}

}  // namespace tcperf
