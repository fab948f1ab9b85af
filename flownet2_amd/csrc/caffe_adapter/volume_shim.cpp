// Test entry of the adapter library (libfn2_caffe_adapter_test.so, build_adapter.sh) for Convolution / Deconvolution layers on blobs of any
// number of axes: `axis`, 0 to 3 spatial axes behind it, the repeated fields given once or once per axis, force_nd_im2col.  The layer is
// created BY TYPE STRING through LayerRegistry -- in this library the plug-ins of fn2_caffe_layers.cpp --, given weights and bias, run forward
// and, on request, backward with the given parameter diffs already in place (the layers accumulate into them).  All pointers are HOST
// pointers.  It compiles no reference source.  tests/test_conv_volume_adapter.py.
#include <cstdio>
#include <cstring>
#include <exception>

#include "caffe/blob.hpp"
#include "caffe/layer.hpp"
#include "caffe/layer_factory.hpp"

using namespace caffe;

// The layer description, `layer`: {deconv, num_output, group, axis, force_nd_im2col, bottom axes A, n_kernel, n_stride, n_pad, n_dilation}
// followed by the A bottom extents and the n_kernel + n_stride + n_pad + n_dilation entries of the four repeated fields, as a prototxt would
// state them.  top may be NULL (top_shape alone is wanted); top_shape holds top_axes extents on return, at most 8.  backward != 0: top_diff,
// weight_diff0 (and bias_diff0 with a bias) in, bottom_diff, weight_diff (and bias_diff) out.  Returns 0, or -1 with the exception's text in err.
extern "C" __attribute__((visibility("default")))
int fn2_adapter_volume_layer(const int* layer, const float* x, const float* weight, int weight_count, const float* bias /* nullable: bias_term false */,
                             float* top /* nullable */, int* top_shape /* [8] */, int* top_axes, int* weight_shape /* [8] */, int* weight_axes, int backward,
                             const float* top_diff, const float* weight_diff0, const float* bias_diff0, float* bottom_diff, float* weight_diff,
                             float* bias_diff, char* err, int err_len) {
  try {
    Caffe::set_mode(Caffe::GPU);
    const int deconv = layer[0], num_output = layer[1], axes = layer[5];
    LayerParameter lp;
    lp.set_name("volume_under_test");
    lp.set_type(deconv ? "Deconvolution" : "Convolution");
    ConvolutionParameter* cp = lp.mutable_convolution_param();
    cp->set_num_output(num_output);
    cp->set_bias_term(bias != nullptr);
    cp->set_group(layer[2]);
    cp->set_axis(layer[3]);
    cp->set_force_nd_im2col(layer[4] != 0);
    const int* v = layer + 10;
    const vector<int> shape(v, v + axes);
    v += axes;
    for (int i = 0; i < layer[6]; ++i) cp->add_kernel_size(*v++);
    for (int i = 0; i < layer[7]; ++i) cp->add_stride(*v++);
    for (int i = 0; i < layer[8]; ++i) cp->add_pad(*v++);
    for (int i = 0; i < layer[9]; ++i) cp->add_dilation(*v++);
    cp->mutable_weight_filler()->set_type("constant");
    cp->mutable_bias_filler()->set_type("constant");
    shared_ptr<Layer<float> > made = LayerRegistry<float>::CreateLayer(lp);
    Blob<float> bot(shape), out;
    std::memcpy(bot.mutable_cpu_data(), x, sizeof(float) * bot.count());
    vector<Blob<float>*> bottom{&bot}, tops{&out};
    made->SetUp(bottom, tops);
    Blob<float>& w = *made->blobs()[0];
    *weight_axes = w.num_axes();
    for (int i = 0; i < w.num_axes() && i < 8; ++i) weight_shape[i] = w.shape(i);
    CHECK_EQ(w.count(), weight_count) << "the weight blob is not of the size the caller states";
    std::memcpy(w.mutable_cpu_data(), weight, sizeof(float) * w.count());
    if (bias) std::memcpy(made->blobs()[1]->mutable_cpu_data(), bias, sizeof(float) * num_output);
    if (backward) {
      std::memcpy(w.mutable_cpu_diff(), weight_diff0, sizeof(float) * w.count());
      if (bias) std::memcpy(made->blobs()[1]->mutable_cpu_diff(), bias_diff0, sizeof(float) * num_output);
    }
    made->Forward(bottom, tops);
    CHECK_LE(out.num_axes(), 8);
    *top_axes = out.num_axes();
    for (int i = 0; i < out.num_axes(); ++i) top_shape[i] = out.shape(i);
    if (backward) {
      std::memcpy(out.mutable_cpu_diff(), top_diff, sizeof(float) * out.count());
      made->Backward(tops, vector<bool>{true}, bottom);
    }
    CUDA_CHECK(hipDeviceSynchronize());
    if (top) std::memcpy(top, out.cpu_data(), sizeof(float) * out.count());
    if (backward) {
      std::memcpy(bottom_diff, bot.cpu_diff(), sizeof(float) * bot.count());
      std::memcpy(weight_diff, w.cpu_diff(), sizeof(float) * w.count());
      if (bias) std::memcpy(bias_diff, made->blobs()[1]->cpu_diff(), sizeof(float) * num_output);
    }
    return 0;
  } catch (const std::exception& e) {
    if (err && err_len > 0) std::snprintf(err, (size_t)err_len, "%s", e.what());
    return -1;
  }
}
