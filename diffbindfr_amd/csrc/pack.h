// Weight packing: a conv's checkpoint tensors -> the byte layouts k_conv, k_conv2 / k_conv2h and k_convz read (pack.cpp).  Host code only: the
// packers call no HIP function and read no environment variable; api.cpp looks the tensors up, calls them and uploads what they return.
#pragma once
#include "common.h"

// a row of an fp16 tile whose largest magnitude is 2^(15 - d) after the tile's factor has depth d: up to this depth two fp16 pieces keep 22 bits of it (pack_f16_tiles)
#define F16_ROW_DEPTH_OK 17

// The seven tensors of one TensorProductConvLayer: fc.lin.0 (K x K) and fc.lin.3 (W x K) with their biases, batch_norm's three vectors ...
enum ConvTensor { T_W1, T_B1, T_W2, T_B2, T_MEAN_SHIFT, T_AFFINE_WEIGHT, T_AFFINE_BIAS, N_CONV_TENSORS };
struct ConvTensors { const float* p[N_CONV_TENSORS]; };
// ... their names behind the conv's, and their element counts
extern const char* const conv_tensor_suffix[N_CONV_TENSORS];
void conv_tensor_numel(const ConvSpec& sp, int64_t numel[N_CONV_TENSORS]);

// What a packer returns: the scalar fields in `w` (every pointer of it null), the arrays next to it.
struct PackedConv  { ConvW w;  std::vector<float> W1p, b1, W2p, b2p, mean_shift, weight, bias; std::vector<RunDesc> runs; };
struct PackedConv2 { ConvW2 w; bool vector_only; std::vector<float> W2q, b2q, W2rinv, W1rinv; std::vector<uint16_t> W2h, W1h; std::vector<RunDesc> runs; };   // W2rinv / W1rinv: empty without per-row factors
struct PackedConvZ { ConvZ w;  std::vector<uint32_t> cdesc; std::vector<float> rowinv; std::vector<uint16_t> W2z; };

// `name` goes into the error messages (dbfr_set_error); the return value is a DBFR_* status.
int pack_conv(const ConvTensors& t, int kind, const std::string& name, PackedConv* o);
// rowscale (DBFR_F16_ROWSCALE): 0 never packs with per-row factors, 1 packs a conv that way when a run of it is deeper than F16_ROW_DEPTH_OK, 2 always
int pack_conv2(const ConvTensors& t, int kind, const std::string& name, int rowscale, bool vector_only, PackedConv2* o);
int pack_convz(const ConvTensors& t, int kind, const std::string& name, int k1, PackedConvZ* o);   // k1: of the conv's (full) pack_conv2

// f(name, array, the pointer of `w` it belongs to) for every array of a packed conv, in the order model creation uploads them
template <typename F> void each_array(PackedConv& p, F f) {
  f("W1p", p.W1p, p.w.W1p); f("b1", p.b1, p.w.b1); f("W2p", p.W2p, p.w.W2p); f("b2p", p.b2p, p.w.b2p); f("runs", p.runs, p.w.runs);
  f("ln.mean_shift", p.mean_shift, p.w.ln.mean_shift); f("ln.weight", p.weight, p.w.ln.weight); f("ln.bias", p.bias, p.w.ln.bias);
}
template <typename F> void each_array(PackedConv2& p, F f) {
  if (!p.vector_only) { f("W2q", p.W2q, p.w.W2q); f("b2q", p.b2q, p.w.b2q); }
  if (!p.W2rinv.empty()) f("W2rinv", p.W2rinv, p.w.W2rinv);
  f("W2h", p.W2h, p.w.W2h);
  if (!p.W1rinv.empty()) f("W1rinv", p.W1rinv, p.w.W1rinv);
  f("W1h", p.W1h, p.w.W1h); f("runs", p.runs, p.w.runs);
}
template <typename F> void each_array(PackedConvZ& p, F f) {
  f("cdesc", p.cdesc, p.w.cdesc); f("rowinv", p.rowinv, p.w.rowinv); f("W2z", p.W2z, p.w.W2z);
}
