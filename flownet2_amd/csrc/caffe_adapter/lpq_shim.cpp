// Test entry of the adapter library (libfn2_caffe_adapter_test.so, build_adapter.sh) for the LpqLoss plug-in: the layer is created BY
// TYPE STRING through LayerRegistry -- in this library the plug-in of fn2_caffe_layers.cpp --, owned by a net whose iteration the caller
// states, and run forward and backward.  All pointers are HOST pointers.  It compiles no reference source.  tests/test_lpq_loss_adapter.py.
#include <cstdio>
#include <cstring>
#include <exception>

#include "caffe/blob.hpp"
#include "caffe/layer.hpp"
#include "caffe/layer_factory.hpp"
#include "caffe/net.hpp"

using namespace caffe;

// b1 may be NULL (one bottom).  The schedule: nstarts starts, np values of p, nq values of q, as the prototxt would state them.
// flags: bit 0 l2_prescale_by_channels, bit 1 normalize_by_num_entries.  iter < 0: the layer has no net (GetNet() == NULL); otherwise
// net.set_iter(iter) before EVERY one of the `passes` forward + backward passes, with iter advanced by iter_step between them (one layer
// object walks through its schedule).  Outputs of the LAST pass: loss[1], d0 and d1 (d1 nullable) of the bottoms' size.
// Returns 0, or -1 with the exception's text in err.
extern "C" __attribute__((visibility("default")))
int fn2_adapter_lpq_layer(const float* b0, const float* b1, int N, int C, int H, int W, int nstarts, const int* starts, int np, const float* ps,
                          int nq, const float* qs, float p_epsilon, float q_epsilon, int flags, int iter, int iter_step, int passes,
                          float top_diff, float* loss, float* d0, float* d1, char* err, int err_len) {
  try {
    Caffe::set_mode(Caffe::GPU);
    LayerParameter lp;
    lp.set_name("lpq_under_test");
    lp.set_type("LpqLoss");
    LpqLossParameter* pp = lp.mutable_lpq_loss_param();
    for (int i = 0; i < nstarts; ++i) pp->add_pq_episode_starts_at_iter((unsigned)starts[i]);
    for (int i = 0; i < np; ++i) pp->add_p(ps[i]);
    for (int i = 0; i < nq; ++i) pp->add_q(qs[i]);
    pp->set_p_epsilon(p_epsilon);
    pp->set_q_epsilon(q_epsilon);
    pp->set_l2_prescale_by_channels((flags & 1) != 0);
    pp->set_normalize_by_num_entries((flags & 2) != 0);
    shared_ptr<Layer<float> > layer = LayerRegistry<float>::CreateLayer(lp);
    Net<float> net;
    if (iter >= 0) layer->SetNet(&net);
    Blob<float> bot0(N, C, H, W), bot1(N, C, H, W), out;
    std::memcpy(bot0.mutable_cpu_data(), b0, sizeof(float) * bot0.count());
    if (b1) std::memcpy(bot1.mutable_cpu_data(), b1, sizeof(float) * bot1.count());
    vector<Blob<float>*> bottom{&bot0}, tops{&out};
    if (b1) bottom.push_back(&bot1);
    layer->SetUp(bottom, tops);
    for (int k = 0; k < passes; ++k) {
      if (iter >= 0) net.set_iter(iter + k * iter_step);
      layer->Forward(bottom, tops);
      out.mutable_cpu_diff()[0] = top_diff;
      layer->Backward(tops, vector<bool>(bottom.size(), true), bottom);
    }
    CUDA_CHECK(hipDeviceSynchronize());
    loss[0] = out.cpu_data()[0];
    std::memcpy(d0, bot0.cpu_diff(), sizeof(float) * bot0.count());
    if (b1 && d1) std::memcpy(d1, bot1.cpu_diff(), sizeof(float) * bot1.count());
    return 0;
  } catch (const std::exception& e) {
    if (err && err_len > 0) std::snprintf(err, (size_t)err_len, "%s", e.what());
    return -1;
  }
}
