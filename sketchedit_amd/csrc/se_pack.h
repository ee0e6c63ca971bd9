// Internal (host-only) interface of the weight packer (se_pack.hip): the device images a layer holds and the function that
// builds them.  WHICH images a layer gets is layer_facts (se_dispatch.h), the same facts choose_form reads: pack_layer_images
// builds exactly those and checks that it did.
#pragma once
#include <hip/hip_runtime.h>

#include "se_dispatch.h"

#include <cstddef>
#include <string>
#include <vector>

namespace se {

// sole owner of one device allocation (move-only): freed when reallocated, reset or destroyed; reads as the raw pointer
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
    return *this;
  }
  ~DevBuf() { reset(); }
  hipError_t alloc(size_t bytes) { reset(); return hipMalloc(&p_, bytes); }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
  }
  operator float*() const { return p_; }

 private:
  float* p_ = nullptr;
};

struct Layer {
  LayerDef def;
  std::vector<float> w, b;    // host copies in checkpoint layout
  bool have_w = false, have_b = false, packed = false;
  LayerFacts facts = {};      // layer_facts(def, stored channels): the packing numbers and which images below exist
  DevBuf direct[2];           // the image of the direct kernels (gather-GEMM, raw tile), [0] fp32, [1] bf16: facts.nch chunks of
                              //   128-byte rows (32 fp32 or 64 bf16 k-values), same row order and slot swizzle; for a raw layer
                              //   the [cout][9][12] fp32 weights ([1]: rounded to bf16, kept as fp32)
  DevBuf d_b;       // bias in the row order of the direct image (raw layers: as in the checkpoint)
  DevBuf d_u;       // Winograd-transformed weights (eligible layers only)
  DevBuf d_ub;      // bias in the row order of the 48 -> 96 Winograd kernel (MIXED tiles)
  DevBuf d_w16d;    // bf16, 5x5 layers whose stored input has <= 4 real channels: pair-of-taps image (pack_layer16_d4, se_rtile.hip)
  DevBuf d_w16s;    // 96 -> 192 3x3 only: the 32-k step image of the 8 x 16 raw-tile kernel (se_rconv16.hip)
  DevBuf d_w96;     // 96-row stride-1 layers: the 32-k step image of se_rconv96.hip
  DevBuf d_u1;      // two-source 96+96 -> 192 layers: Winograd image of the FIRST source's 96 channels alone, and
  DevBuf d_wv;      //   the second source's direct weights [9 taps][96][192 packed rows] (vector source folded into a bias)
  DevBuf d_wv16;    //   the same rounded to bf16 (kept as fp32 values) for the bf16 mode
  DevBuf d_u24;     // 96 -> 192 3x3: image of the hybrid F(2,3) x F(4,3) kernel (first 96 input channels), se_wino24.hip
  DevBuf d_ub24;    //   and the bias in its MIXED row order
  DevBuf d_u24b;    //   two-source layers: the image over both sources (6 chunks per position)
  DevBuf d_wx;      // 24 -> 24 3x3: image of the F(2,3)-along-x raw-tile kernel (se_rtilew.hip)
  DevBuf d_wx2;     //   and of its two-dimensional F(2x2,3x3) form
  DevBuf d_wd;      // 5x5 layers with padding channels in their stored input (fp32): dense-K image (se_rtile.hip)
  DevBuf d_wdw;     //   and the image of its F(2,5)-along-x form (rtile_dense5w_kernel)
  DevBuf d_s2p;     // 3x3 stride 2, 48 -> 96 / 192 (fp32): polyphase F(2,2) image (se_s2poly.hip)
  DevBuf d_s2pb;    //   and the bias in its MIXED row order
};

// Builds every device image of a layer, in both precisions, from its host weights: those layer_facts names, no other (checked
// before it returns) -- the one rule for which kernel forms a layer can run.  `chans` lists the checkpoint input channels its
// stored input carries, in stored order -- the identity for every layer but the 4-channel form of wconv1.  Returns 1 with the
// reason in `err`.
int pack_layer_images(Layer& L, const std::vector<int>& chans, std::string& err);

}  // namespace se
