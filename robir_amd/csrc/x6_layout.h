// Stream layout of the exact-operand ("f16x6") chunk-stream nets.  A packed blob (packing.pack_*_x6: rb_pack_layer_x6 per layer) is the
// net's layers back to back, a layer = nch(l) chunks of 16 output neurons x K(l) x 3 pieces (sx_cf4(K) float4 each, bias first); the
// kernels walk it as ONE cyclic stream: the chunks behind a round's last are the next round's first.  A net says how many layers it has,
// K(l) and nch(l); SxStream derives the rest.  One- and two-tile forms of a net share its description.
#pragma once
#include "x6_ring.h"

namespace rb {

template <class Net>
struct SxStream {
  __host__ __device__ static constexpr int nchunk() { return cbase(Net::NL); }
  __host__ __device__ static constexpr int cbase(int l) {             // first chunk of layer l
    int n = 0;
    for (int i = 0; i < l; ++i) n += Net::nch(i);
    return n;
  }
  __host__ __device__ static constexpr int layer_of(int c) {          // stream position (may run past the end once: cyclic) -> layer
    if (c >= nchunk()) c -= nchunk();
    int l = 0, first = 0;
    for (int i = 0; i < Net::NL - 1; ++i) {
      first += Net::nch(i);
      if (c >= first) l = i + 1;
    }
    return l;
  }
  __host__ __device__ static constexpr int nruns() {                  // runs of layers with chunks of one size
    int n = 1;
    for (int l = 1; l < Net::NL; ++l) n += Net::K(l) != Net::K(l - 1);
    return n;
  }
  // float4 offset of chunk c (cyclic) in the packed blob.  Two spellings of one function: the optimiser does not turn the walk over the
  // layers into the closed form of a net with one or two runs, and the two-tile kernels sit at the edge of the register file -- a
  // different scalar sequence here moves their spills (profiles/x6_engine_refactor.md).
  __host__ __device__ static constexpr long coff(int c) {
    if (c >= nchunk()) c -= nchunk();
    if (nruns() <= 2) {
      long off = (long)c * sx_cf4(Net::K(0));
      for (int l = 1; l < Net::NL; ++l)
        if (Net::K(l) != Net::K(l - 1) && c >= cbase(l)) off = loff(l) + (long)(c - cbase(l)) * sx_cf4(Net::K(l));
      return off;
    }
    long off = 0;
    int first = 0, base = 0, kl = Net::K(0);
    for (int i = 0; i < Net::NL - 1; ++i) {
      first += Net::nch(i);
      if (c >= first) {
        off += (long)Net::nch(i) * sx_cf4(Net::K(i));
        base = first;
        kl = Net::K(i + 1);
      }
    }
    return off + (long)(c - base) * sx_cf4(kl);
  }
  __host__ __device__ static constexpr long loff(int l) {             // ... of layer l's first chunk
    long off = 0;
    for (int i = 0; i < l; ++i) off += (long)Net::nch(i) * sx_cf4(Net::K(i));
    return off;
  }
  // layer_of and coff (whichever spelling the net takes) against their definition at every stream position, and past the end
  __host__ __device__ static constexpr bool consistent() {
    for (int c = 0; c < nchunk() + 3; ++c) {
      const int cc = c >= nchunk() ? c - nchunk() : c, l = layer_of(c);
      if (cc < cbase(l) || cc >= cbase(l) + Net::nch(l)) return false;
      if (coff(c) != loff(l) + (long)(cc - cbase(l)) * sx_cf4(Net::K(l))) return false;
    }
    return true;
  }
};

// NeuS SDF net (packing.pack_sdf_x6; sdf_x6.hip, sdf_x6t.hip): nine layers, K padded to 64, 256 x3, 288 = [208 | 64 | 16 zero], 256 x4;
// LAST = chunks of the output layer: 17 (all 257 outputs) or 1 (signed distance only)
constexpr int SX_SLOT_B = 27 * 1024 + 512;      // K = 288: 27 KB of fragments (+ slack: the slot's last copy may start 1 KB early)
template <int LAST>
struct SxSdfNet {
  static constexpr int NL = 9;
  __host__ __device__ static constexpr int K(int l) { return l == 0 ? 64 : (l == 4 ? 288 : 256); }
  __host__ __device__ static constexpr int nch(int l) { return l == 3 ? 13 : (l == 8 ? LAST : 16); }
};
// NeuS colour net (packing.pack_color_x6; color_x6.hip, color_x6t.hip): K = 320 for the first layer, 256 after, one output chunk
struct SxColorNet {
  static constexpr int NL = 5;
  __host__ __device__ static constexpr int K(int l) { return l == 0 ? 320 : 256; }
  __host__ __device__ static constexpr int nch(int l) { return l == 4 ? 1 : 16; }
};
// visibility net (packing.pack_vis_x6; vis_x6.hip): the colour net's shape with K = 128 for the first layer
struct SxVisNet {
  static constexpr int NL = 5;
  __host__ __device__ static constexpr int K(int l) { return l == 0 ? 128 : 256; }
  __host__ __device__ static constexpr int nch(int l) { return l == 4 ? 1 : 16; }
};
// the SDF net back to front (packing.pack_sdf_back_x6; sdf_back_x6.hip has the table): W7^T .. W0^T, layer 3 with the four skip chunks,
// W3^T with K4 = 224 = 208 + 16 zero; K4 = 256: the two-tile form's blob (sdf_back_x6t.hip), every layer at K = 256
template <int K4>
struct SxSdfBackNet {
  static constexpr int NL = 8;
  __host__ __device__ static constexpr int K(int l) { return l == 4 ? K4 : 256; }
  __host__ __device__ static constexpr int nch(int l) { return l == 3 ? 17 : (l == 7 ? 4 : 16); }
};

static_assert(SxStream<SxSdfNet<17>>::consistent() && SxStream<SxSdfNet<1>>::consistent() && SxStream<SxColorNet>::consistent() &&
                  SxStream<SxVisNet>::consistent() && SxStream<SxSdfBackNet<224>>::consistent() && SxStream<SxSdfBackNet<256>>::consistent(),
              "coff / layer_of disagree with the layer table");
static_assert(SxStream<SxSdfNet<17>>::nchunk() == 142 && SxStream<SxSdfNet<1>>::nchunk() == 126, "");
static_assert(SxStream<SxSdfNet<17>>::coff(141) == 201780 && SxStream<SxSdfNet<1>>::coff(125) == 177140, "");
static_assert(SxStream<SxColorNet>::nchunk() == 65 && SxStream<SxColorNet>::coff(64) == 104704, "");
static_assert(SxStream<SxVisNet>::nchunk() == 65 && SxStream<SxVisNet>::coff(64) == 86272, "");
static_assert(SxStream<SxSdfBackNet<224>>::nchunk() == 117 && SxStream<SxSdfBackNet<224>>::coff(116) == 175568, "");
static_assert(SxStream<SxSdfBackNet<256>>::nchunk() == 117 && SxStream<SxSdfBackNet<256>>::coff(116) == 116L * sx_cf4(256), "");
static_assert(SxStream<SxSdfNet<17>>::layer_of(141 + 3) == 0 && SxStream<SxSdfNet<17>>::layer_of(61) == 4, "the stream is cyclic");

}  // namespace rb
