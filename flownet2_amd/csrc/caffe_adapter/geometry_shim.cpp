// Test entry of the adapter library (libfn2_caffe_adapter_test.so, build_adapter.sh) for Convolution / Deconvolution layers with
// rectangular taps, per-axis stride / pad / dilation and groups: the layer is created BY TYPE STRING through LayerRegistry -- in this
// library the plug-ins of fn2_caffe_layers.cpp --, given weights and bias, run forward and, on request, backward with the given parameter
// diffs already in place (the layers accumulate into them).  All pointers are HOST pointers.  tests/test_conv_geometry_adapter.py.
#include <cstdio>
#include <cstring>
#include <exception>

#include "caffe/blob.hpp"
#include "caffe/layer.hpp"
#include "caffe/layer_factory.hpp"

using namespace caffe;

// taps: {kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group}.  A pair of equal values is stated the
// short way (one repeated entry), a pair of different values the long way (kernel_h / kernel_w, ..., two dilation entries), so both
// readings of LayerSetUp are used.  top may be NULL (top_shape alone is wanted).  backward != 0: top_diff, weight_diff0 (and bias_diff0
// with a bias) in, bottom_diff, weight_diff (and bias_diff) out.  Returns 0, or -1 with the exception's text in err.
extern "C" __attribute__((visibility("default")))
int fn2_adapter_geometry_layer(int deconv, const int* taps, int num_output, const float* x, int N, int C, int H, int W, const float* weight,
                               int weight_count, const float* bias /* nullable: bias_term false */, float* top /* nullable */, int* top_shape /* [4] */,
                               int backward, const float* top_diff, const float* weight_diff0, const float* bias_diff0, float* bottom_diff,
                               float* weight_diff, float* bias_diff, char* err, int err_len) {
  try {
    Caffe::set_mode(Caffe::GPU);
    LayerParameter lp;
    lp.set_name("geometry_under_test");
    lp.set_type(deconv ? "Deconvolution" : "Convolution");
    ConvolutionParameter* cp = lp.mutable_convolution_param();
    cp->set_num_output(num_output);
    cp->set_bias_term(bias != nullptr);
    if (taps[0] == taps[1]) cp->add_kernel_size(taps[0]); else { cp->set_kernel_h(taps[0]); cp->set_kernel_w(taps[1]); }
    if (taps[2] == taps[3]) cp->add_stride(taps[2]); else { cp->set_stride_h(taps[2]); cp->set_stride_w(taps[3]); }
    if (taps[4] == taps[5]) cp->add_pad(taps[4]); else { cp->set_pad_h(taps[4]); cp->set_pad_w(taps[5]); }
    cp->add_dilation(taps[6]);
    if (taps[6] != taps[7]) cp->add_dilation(taps[7]);
    cp->set_group(taps[8]);
    cp->mutable_weight_filler()->set_type("constant");
    cp->mutable_bias_filler()->set_type("constant");
    shared_ptr<Layer<float> > layer = LayerRegistry<float>::CreateLayer(lp);
    Blob<float> bot(N, C, H, W), out;
    std::memcpy(bot.mutable_cpu_data(), x, sizeof(float) * bot.count());
    vector<Blob<float>*> bottom{&bot}, tops{&out};
    layer->SetUp(bottom, tops);
    Blob<float>& w = *layer->blobs()[0];
    CHECK_EQ(w.count(), weight_count) << "the weight blob is not of the size the caller states";
    std::memcpy(w.mutable_cpu_data(), weight, sizeof(float) * w.count());
    if (bias) std::memcpy(layer->blobs()[1]->mutable_cpu_data(), bias, sizeof(float) * num_output);
    if (backward) {
      std::memcpy(w.mutable_cpu_diff(), weight_diff0, sizeof(float) * w.count());
      if (bias) std::memcpy(layer->blobs()[1]->mutable_cpu_diff(), bias_diff0, sizeof(float) * num_output);
    }
    layer->Forward(bottom, tops);
    for (int i = 0; i < 4; ++i) top_shape[i] = out.shape(i);
    if (backward) {
      std::memcpy(out.mutable_cpu_diff(), top_diff, sizeof(float) * out.count());
      layer->Backward(tops, vector<bool>{true}, bottom);
    }
    CUDA_CHECK(hipDeviceSynchronize());
    if (top) std::memcpy(top, out.cpu_data(), sizeof(float) * out.count());
    if (backward) {
      std::memcpy(bottom_diff, bot.cpu_diff(), sizeof(float) * bot.count());
      std::memcpy(weight_diff, w.cpu_diff(), sizeof(float) * w.count());
      if (bias) std::memcpy(bias_diff, layer->blobs()[1]->cpu_diff(), sizeof(float) * num_output);
    }
    return 0;
  } catch (const std::exception& e) {
    if (err && err_len > 0) std::snprintf(err, (size_t)err_len, "%s", e.what());
    return -1;
  }
}
