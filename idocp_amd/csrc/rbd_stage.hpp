// Layout of one host-pointer call of the batched rigid-body API (rbd_capi.hip) in the handle's staging buffer: which arrays get room, where,
// what is copied up before the launches and what comes back after them.  Plain C++17 without a HIP call, so that a CPU program can hold the
// layout to its rules (tests/cpp/rbd_stage_layout.cpp); rbd_capi.hip walks the three lists with hipMemcpyAsync / hipMemsetAsync.
//
// A slot is declared from a host pointer, a size in doubles and the place that receives its device pointer.  A null pointer or a size of zero
// takes no room and gives a null device pointer.  Slots lie behind one another, each at an even number of doubles (16 bytes) from the base.
#pragma once

#include <cstddef>

namespace idocp_host {

struct StagePlan {
  struct Copy { double* host; size_t offset, count; };      // `count` doubles between host memory and base + offset
  static constexpr int MAX_SLOTS = 24;                      // (the largest call, idocp_rbd_ilqr_accept, declares 19)
  Copy up[MAX_SLOTS], down[MAX_SLOTS], zero[MAX_SLOTS];     // host to device; device to host; zero-filled before the launch (host: null)
  int n_up = 0, n_down = 0, n_zero = 0, n_slots = 0;

  size_t total() const { return total_; }                   // doubles of the buffer

  // uploaded in full
  void in(const double* host, size_t size, const double** dev) { add(const_cast<double*>(host), host ? size : 0, size, size, false, dev); }
  // downloaded in full
  void out(double* host, size_t size, double** dev, bool zero_fill = false) { add(host, host ? size : 0, 0, 0, zero_fill, constPtr(dev)); }
  // the first `prefix` doubles go up, the rest comes back (a trajectory whose slice 0 is the input)
  void inout(double* host, size_t size, size_t prefix, double** dev) { add(host, host ? size : 0, prefix, prefix, false, constPtr(dev)); }
  // the first `prefix` doubles go up, everything comes back (a trajectory whose slice 0 is an input the call rewrites as well)
  void inoutAll(double* host, size_t size, size_t prefix, double** dev) { add(host, host ? size : 0, prefix, 0, false, constPtr(dev)); }
  // uploaded in full and downloaded in full (sums a call adds to)
  void update(double* host, size_t size, double** dev) { add(host, host ? size : 0, size, 0, false, constPtr(dev)); }
  // room without a copy
  void deviceOnly(size_t size, double** dev) { add(nullptr, size, 0, size, false, constPtr(dev)); }

  // hands every declared slot its device pointer
  void bind(double* base) const { for (int i = 0; i < n_slots; ++i) *slot_[i].dev = base + slot_[i].offset; }

 private:
  struct Slot { const double** dev; size_t offset; };
  Slot slot_[MAX_SLOTS];
  size_t total_ = 0;

  static const double** constPtr(double** p) { return const_cast<const double**>(p); }

  // size 0: absent; [0, upload) goes up, [download_from, size) comes back
  void add(double* host, size_t size, size_t upload, size_t download_from, bool zero_fill, const double** dev) {
    *dev = nullptr;
    if (!size) return;
    const size_t at = total_;
    if (upload) up[n_up++] = {host, at, upload};
    if (download_from < size) down[n_down++] = {host + download_from, at + download_from, size - download_from};
    if (zero_fill) zero[n_zero++] = {nullptr, at, size};
    slot_[n_slots++] = {dev, at};
    total_ += (size + 1) / 2 * 2;
  }
};

}  // namespace idocp_host
