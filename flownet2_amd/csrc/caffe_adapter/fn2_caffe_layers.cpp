// Caffe adapter: the FlowNet2 custom layers as `caffe::Layer<float>` plug-ins whose Forward_gpu / Backward_gpu
// call libflownet2_hip.so (the C ABI in include/flownet2_hip.h) with the Blobs' device pointers.
//
// How a maintainer of the reference uses it: drop this file into src/caffe/layers/, REMOVE the
// reference's correlation_layer.{cpp,cu}, flow_warp_layer.{cpp,cu}, resample_layer.{cpp,cu}, l1loss_layer.{cpp,cu},
// channel_norm_layer.{cpp,cu}, downsample_layer.{cpp,cu} from the build (a type string can only be registered
// once, layer_factory.hpp:69-70), build Caffe for ROCm and link -lflownet2_hip.  Prototxts and .caffemodel files
// are untouched: same `type:` strings, same *_param fields, same blob shapes.
//
// In this repository the file is compiled against the stand-in headers in compat/ (no Caffe tree exists here),
// and the resulting plug-ins are driven through LayerRegistry exactly like the reference's own classes
// (tests/test_caffe_adapter.py compares the two side by side on the GPU).
//
// Class and member names follow the reference headers (include/caffe/layers/correlation_layer.hpp:26-77,
// flow_warp_layer.hpp, l1_loss_layer.hpp, channel_norm_layer.hpp, downsample_layer.hpp,
// src/caffe/layers/resample_layer.hpp) so that the class is recognisable; the bodies are new.
// Only Dtype = float is instantiated: the C ABI is fp32 (the reference's tools use float, tools/caffe.cpp:203).
#include <algorithm>
#include <cmath>
#include <sstream>
#include <type_traits>
#include <vector>

#include "caffe/blob.hpp"
#include "caffe/filler.hpp"
#include "caffe/layer.hpp"
#include "caffe/layer_factory.hpp"
#include "caffe/net.hpp"
#include "caffe/proto/caffe.pb.h"

#include "flownet2_hip.h"
#include "flownet2_hip_conv_volume.h"
#include "flownet2_hip_lpq_loss.h"

namespace caffe {

#define FN2_CALL(expr)                                                                  \
  do {                                                                                  \
    const int fn2_rc_ = (expr);                                                         \
    if (fn2_rc_ != FN2_OK) LOG(FATAL) << #expr << " -> " << fn2_rc_ << ": " << fn2_last_error_string(); \
  } while (0)

// The C ABI is fp32.  In a real Caffe build INSTANTIATE_CLASS also instantiates Dtype = double
// (common.hpp:41-66); those instantiations must compile but abort if they are ever run.
template <typename Dtype> static inline const float* f32(const Dtype* p) {
  if constexpr (std::is_same<Dtype, float>::value) { return p; }
  else { LOG(FATAL) << "flownet2_hip layers are fp32 only (Dtype = double requested)"; return nullptr; }
}
template <typename Dtype> static inline float* f32(Dtype* p) {
  if constexpr (std::is_same<Dtype, float>::value) { return p; }
  else { LOG(FATAL) << "flownet2_hip layers are fp32 only (Dtype = double requested)"; return nullptr; }
}

// All reference launches go to the legacy default stream (no stream argument anywhere in the fork); so do we.
static void* const kStream = nullptr;

// ---------------------------------------------------------------------------------------------------------
template <typename Dtype>
class CorrelationLayer : public Layer<Dtype> {
 public:
  explicit CorrelationLayer(const LayerParameter& param) : Layer<Dtype>(param) {}
  virtual void LayerSetUp(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    const CorrelationParameter& cp = this->layer_param_.correlation_param();
    CHECK(cp.has_kernel_size()) << "Filter kernel_size is not set";
    CHECK(cp.has_max_displacement()) << "Max displacement is required.";
    if (cp.kernel_size() % 2 == 0) LOG(FATAL) << "Odd kernel size required";
    params_.pad = cp.pad();
    params_.kernel_size = cp.kernel_size();
    params_.max_displacement = cp.max_displacement();
    params_.stride1 = cp.stride_1();
    params_.stride2 = cp.stride_2();
    params_.corr_type = cp.correlation_type() == CorrelationParameter_CorrelationType_SUBTRACT ? FN2_CORR_SUBTRACT : FN2_CORR_MULTIPLY;
    params_.do_abs = cp.do_abs();
    params_.single_direction = 0;   // Correlation1D only
  }
  virtual void Reshape(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    CHECK_EQ(bottom[0]->width(), bottom[1]->width()) << "Both bottom blobs must have same width";
    CHECK_EQ(bottom[0]->height(), bottom[1]->height()) << "Both bottom blobs must have same height";
    CHECK_EQ(bottom[0]->channels(), bottom[1]->channels()) << "Both bottom blobs must have same height";
    num_ = bottom[0]->num();
    FN2_CALL(fn2_correlation_out_shape(&params_, bottom[0]->channels(), bottom[0]->height(), bottom[0]->width(),
                                       &top_channels_, &top_height_, &top_width_));
    top[0]->Reshape(num_, top_channels_, top_height_, top_width_);
    // no rbot1_/rbot2_/rtopdiff_ scratch: the kernels read NCHW directly
  }
  virtual inline const char* type() const { return "Correlation"; }
  virtual inline int ExactNumBottomBlobs() const { return 2; }
  virtual inline int ExactNumTopBlobs() const { return 1; }

 protected:
  virtual void Forward_cpu(const vector<Blob<Dtype>*>&, const vector<Blob<Dtype>*>&) { NOT_IMPLEMENTED; }
  virtual void Backward_cpu(const vector<Blob<Dtype>*>&, const vector<bool>&, const vector<Blob<Dtype>*>&) { NOT_IMPLEMENTED; }
  virtual void Forward_gpu(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    CHECK_EQ(bottom.size(), 2u);
    CHECK_EQ(top.size(), 1u);
    FN2_CALL(fn2_correlation_forward(&params_, f32(bottom[0]->gpu_data()), f32(bottom[1]->gpu_data()), f32(top[0]->mutable_gpu_data()),
                                     bottom[0]->num(), bottom[0]->channels(), bottom[0]->height(), bottom[0]->width(),
                                     nullptr, 0, kStream));
  }
  virtual void Backward_gpu(const vector<Blob<Dtype>*>& top, const vector<bool>&, const vector<Blob<Dtype>*>& bottom) {
    // like the reference: both diffs are always written, propagate_down is ignored
    FN2_CALL(fn2_correlation_backward(&params_, f32(bottom[0]->gpu_data()), f32(bottom[1]->gpu_data()), f32(top[0]->gpu_diff()),
                                      f32(bottom[0]->mutable_gpu_diff()), f32(bottom[1]->mutable_gpu_diff()),
                                      bottom[0]->num(), bottom[0]->channels(), bottom[0]->height(), bottom[0]->width(),
                                      nullptr, 0, kStream));
  }
  fn2_corr_params params_;
  int num_, top_height_, top_width_, top_channels_;
};

// ---------------------------------------------------------------------------------------------------------
// Correlation1D (horizontal displacements; correlation_layer1d.cpp / .cu of the reference)
template <typename Dtype>
class Correlation1DLayer : public Layer<Dtype> {
 public:
  explicit Correlation1DLayer(const LayerParameter& param) : Layer<Dtype>(param) {}
  virtual void LayerSetUp(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    const CorrelationParameter& cp = this->layer_param_.correlation_param();
    CHECK(cp.has_kernel_size()) << "Filter kernel_size is not set";
    CHECK(cp.has_max_displacement()) << "Max displacement is required.";
    if (cp.kernel_size() % 2 == 0) LOG(FATAL) << "Odd kernel size required";
    if (cp.single_direction() < -1 || cp.single_direction() > 1) LOG(FATAL) << "single_direction must be -1 (left), 0 (off), or 1 (right)";
    params_.pad = cp.pad();
    params_.kernel_size = cp.kernel_size();
    params_.max_displacement = cp.max_displacement();
    params_.stride1 = cp.stride_1();
    params_.stride2 = cp.stride_2();
    params_.corr_type = cp.correlation_type() == CorrelationParameter_CorrelationType_SUBTRACT ? FN2_CORR_SUBTRACT : FN2_CORR_MULTIPLY;
    params_.do_abs = cp.do_abs();
    params_.single_direction = cp.single_direction();
  }
  virtual void Reshape(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    CHECK_EQ(bottom[0]->width(), bottom[1]->width()) << "Both bottom blobs must have same width";
    CHECK_EQ(bottom[0]->height(), bottom[1]->height()) << "Both bottom blobs must have same height";
    CHECK_EQ(bottom[0]->channels(), bottom[1]->channels()) << "Both bottom blobs must have same number of channels";
    int tc, th, tw;
    FN2_CALL(fn2_correlation1d_out_shape(&params_, bottom[0]->channels(), bottom[0]->height(), bottom[0]->width(), &tc, &th, &tw));
    top[0]->Reshape(bottom[0]->num(), tc, th, tw);
  }
  virtual inline const char* type() const { return "Correlation1D"; }
  virtual inline int ExactNumBottomBlobs() const { return 2; }
  virtual inline int ExactNumTopBlobs() const { return 1; }

 protected:
  virtual void Forward_cpu(const vector<Blob<Dtype>*>&, const vector<Blob<Dtype>*>&) { NOT_IMPLEMENTED; }
  virtual void Backward_cpu(const vector<Blob<Dtype>*>&, const vector<bool>&, const vector<Blob<Dtype>*>&) { NOT_IMPLEMENTED; }
  virtual void Forward_gpu(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    CHECK_EQ(bottom.size(), 2u);
    CHECK_EQ(top.size(), 1u);
    FN2_CALL(fn2_correlation1d_forward(&params_, f32(bottom[0]->gpu_data()), f32(bottom[1]->gpu_data()), f32(top[0]->mutable_gpu_data()),
                                       bottom[0]->num(), bottom[0]->channels(), bottom[0]->height(), bottom[0]->width(), kStream));
  }
  virtual void Backward_gpu(const vector<Blob<Dtype>*>& top, const vector<bool>&, const vector<Blob<Dtype>*>& bottom) {
    FN2_CALL(fn2_correlation1d_backward(&params_, f32(bottom[0]->gpu_data()), f32(bottom[1]->gpu_data()), f32(top[0]->gpu_diff()),
                                        f32(bottom[0]->mutable_gpu_diff()), f32(bottom[1]->mutable_gpu_diff()),
                                        bottom[0]->num(), bottom[0]->channels(), bottom[0]->height(), bottom[0]->width(), kStream));
  }
  fn2_corr_params params_;
};

// ---------------------------------------------------------------------------------------------------------
// FlowAugmentation (flow_augmentation_layer.cpp / .cu of the reference): the coefficient blobs are read on the host, as there.
template <typename Dtype>
class FlowAugmentationLayer : public Layer<Dtype> {
 public:
  explicit FlowAugmentationLayer(const LayerParameter& param) : Layer<Dtype>(param) {}
  virtual void LayerSetUp(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    CHECK_GT(this->layer_param_.augmentation_param().crop_width(), 0u) << "Please enter crop width if you want to perform augmentation";
    CHECK_GT(this->layer_param_.augmentation_param().crop_height(), 0u) << "Please enter crop height if you want to perform augmentation";
    this->layer_param_.set_reshape_every_iter(false);
  }
  virtual void Reshape(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    CHECK_EQ(bottom.size(), 3u) << "Flow augmentation layer takes three input blobs: FlowField, Img1TransfParams, Img2TransfParams";
    CHECK_EQ(top.size(), 1u) << "Flow augmentation layer outputs one output blob: Augmented Flow";
    CHECK_EQ(bottom[0]->channels(), 2) << "Flow data must have two channels";
    cropped_width_ = this->layer_param_.augmentation_param().crop_width();
    cropped_height_ = this->layer_param_.augmentation_param().crop_height();
    top[0]->Reshape(bottom[0]->num(), 2, cropped_height_, cropped_width_);
  }
  virtual inline const char* type() const { return "FlowAugmentation"; }
  virtual inline bool AllowBackward() const { return false; }

 protected:
  virtual void Forward_cpu(const vector<Blob<Dtype>*>&, const vector<Blob<Dtype>*>&) { LOG(FATAL) << "Forward CPU Augmentation not implemented."; }
  virtual void Backward_cpu(const vector<Blob<Dtype>*>&, const vector<bool>&, const vector<Blob<Dtype>*>&) { LOG(FATAL) << "FlowAugmentationLayer cannot do backward."; }
  virtual void Backward_gpu(const vector<Blob<Dtype>*>&, const vector<bool>&, const vector<Blob<Dtype>*>&) { LOG(FATAL) << "FlowAugmentationLayer cannot do backward."; }
  virtual void Forward_gpu(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    CHECK_EQ(bottom[1]->count() / bottom[0]->num(), FN2_AUG_NUM_PARAMS) << "coefficient blob does not hold one AugmentationCoeff per sample";
    CHECK_EQ(bottom[2]->count(), bottom[1]->count());
    FN2_CALL(fn2_flow_augmentation_forward(f32(bottom[0]->gpu_data()), f32(bottom[1]->cpu_data()), f32(bottom[2]->cpu_data()),
                                           f32(top[0]->mutable_gpu_data()), bottom[0]->num(), bottom[0]->height(), bottom[0]->width(),
                                           cropped_height_, cropped_width_, kStream));
  }
  int cropped_height_, cropped_width_;
};

// ---------------------------------------------------------------------------------------------------------
template <typename Dtype>
class FlowWarpLayer : public Layer<Dtype> {
 public:
  explicit FlowWarpLayer(const LayerParameter& param) : Layer<Dtype>(param) {}
  virtual void Reshape(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    CHECK_EQ(bottom.size(), 2u) << "FlowWarpLayer takes two input blobs: image and flow.";
    CHECK_EQ(top.size(), 1u) << "FlowWarpLayer outputs one blob.";
    CHECK_EQ(bottom[0]->num(), bottom[1]->num()) << "Num of the inputs should be the same";
    CHECK_EQ(2, bottom[1]->channels()) << "Flow should have 2 channels: x-flow and y-flow";
    CHECK_EQ(bottom[0]->width(), bottom[1]->width()) << "Width of the inputs should be the same";
    CHECK_EQ(bottom[0]->height(), bottom[1]->height()) << "Height of the inputs should be the same";
    top[0]->Reshape(bottom[0]->num(), bottom[0]->channels(), bottom[0]->height(), bottom[0]->width());
  }
  virtual inline const char* type() const { return "FlowWarp"; }

 protected:
  virtual void Forward_cpu(const vector<Blob<Dtype>*>&, const vector<Blob<Dtype>*>&) { NOT_IMPLEMENTED; }
  virtual void Backward_cpu(const vector<Blob<Dtype>*>&, const vector<bool>&, const vector<Blob<Dtype>*>&) { NOT_IMPLEMENTED; }
  virtual void Forward_gpu(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    const int fill = this->layer_param_.flow_warp_param().fill_value() == FlowWarpParameter_FillParameter_ZERO ? FN2_FILL_ZERO : FN2_FILL_NAN;
    FN2_CALL(fn2_flow_warp_forward(f32(bottom[0]->gpu_data()), f32(bottom[1]->gpu_data()), f32(top[0]->mutable_gpu_data()), top[0]->num(),
                                   top[0]->channels(), top[0]->height(), top[0]->width(), fill, kStream));
  }
  virtual void Backward_gpu(const vector<Blob<Dtype>*>& top, const vector<bool>& propagate_down, const vector<Blob<Dtype>*>& bottom) {
    // scratch for the inverted scatter (replaces the reference's transposed_image_ blob, flow_warp_layer.cpp:50)
    const size_t ws_bytes = fn2_flow_warp_backward_workspace_bytes(top[0]->num(), top[0]->channels(), top[0]->height(), top[0]->width());
    workspace_.Reshape(vector<int>{(int)((ws_bytes + sizeof(Dtype) - 1) / sizeof(Dtype))});
    FN2_CALL(fn2_flow_warp_backward(f32(bottom[0]->gpu_data()), f32(bottom[1]->gpu_data()), f32(top[0]->gpu_diff()), f32(bottom[0]->mutable_gpu_diff()),
                                    f32(bottom[1]->mutable_gpu_diff()), top[0]->num(), top[0]->channels(), top[0]->height(),
                                    top[0]->width(), propagate_down[0], propagate_down[1], workspace_.mutable_gpu_data(),
                                    workspace_.count() * sizeof(Dtype), kStream));
  }
  Blob<Dtype> workspace_;
};

// ---------------------------------------------------------------------------------------------------------
template <typename Dtype>
class ResampleLayer : public Layer<Dtype> {
 public:
  explicit ResampleLayer(const LayerParameter& param) : Layer<Dtype>(param) {}
  virtual void LayerSetUp(const vector<Blob<Dtype>*>&, const vector<Blob<Dtype>*>&) {
    const ResampleParameter_ResampleType t = this->layer_param().resample_param().type();
    if (t != ResampleParameter_ResampleType_CUBIC && t != ResampleParameter_ResampleType_LINEAR && t != ResampleParameter_ResampleType_NEAREST)
      LOG(FATAL) << "ResampleLayer: only CUBIC, LINEAR and NEAREST interpolation is supported for now";
  }
  virtual void Reshape(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    this->layer_param_.set_reshape_every_iter(false);
    LOG(WARNING) << "ResampleLayer only runs Reshape on setup";
    CHECK_GE(bottom.size(), 1u);
    CHECK_LE(bottom.size(), 2u);
    CHECK_EQ(top.size(), 1u);
    int top_height, top_width;
    if (bottom.size() == 1) {
      top_height = this->layer_param_.resample_param().height();
      top_width = this->layer_param_.resample_param().width();
    } else {
      top_height = bottom[1]->height();
      top_width = bottom[1]->width();
    }
    CHECK_GE(top_height, 1) << "ResampleLayer must have top_height > 0";
    CHECK_GE(top_width, 1) << "ResampleLayer must have top_width > 0";
    top[0]->Reshape(bottom[0]->num(), bottom[0]->channels(), top_height, top_width);
  }
  virtual inline int MinBottomBlobs() const { return 1; }
  virtual inline int MaxBottomBlobs() const { return 2; }
  virtual inline int ExactNumTopBlobs() const { return 1; }
  virtual inline bool AllowBackward() const { LOG(WARNING) << "ResampleLayer does not do backward."; return false; }

 protected:
  virtual void Forward_cpu(const vector<Blob<Dtype>*>&, const vector<Blob<Dtype>*>&) { LOG(FATAL) << "ResampleLayer: CPU Forward not yet implemented."; }
  virtual void Backward_cpu(const vector<Blob<Dtype>*>&, const vector<bool>&, const vector<Blob<Dtype>*>&) { LOG(FATAL) << "ResampleLayer cannot do backward."; }
  virtual void Forward_gpu(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    CHECK_EQ(top[0]->channels(), bottom[0]->channels()) << "ResampleLayer top channel count must match bottom channel count";
    const ResampleParameter& rp = this->layer_param().resample_param();
    FN2_CALL(fn2_resample_forward(f32(bottom[0]->gpu_data()), f32(top[0]->mutable_gpu_data()), bottom[0]->num(), bottom[0]->channels(),
                                  bottom[0]->height(), bottom[0]->width(), top[0]->height(), top[0]->width(), (int)rp.type(),
                                  rp.antialias(), kStream));
  }
  virtual void Backward_gpu(const vector<Blob<Dtype>*>&, const vector<bool>& propagate_down, const vector<Blob<Dtype>*>&) {
    for (size_t i = 0; i < propagate_down.size(); i++)
      if (propagate_down[i]) LOG(FATAL) << "ResampleLayer cannot do backward.";
  }
};

// ---------------------------------------------------------------------------------------------------------
template <typename Dtype>
class L1LossLayer : public Layer<Dtype> {
 public:
  explicit L1LossLayer(const LayerParameter& param) : Layer<Dtype>(param) {}
  virtual void LayerSetUp(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    if (this->layer_param_.loss_weight_size() == 0) this->layer_param_.add_loss_weight(Dtype(1));   // LossLayer::LayerSetUp, loss_layer.cpp:8-13
    if (bottom.size() != 1 && bottom.size() != 2) LOG(FATAL) << "L1LossLayer needs one or two input blobs.";
    const L1LossParameter& lp = this->layer_param_.l1_loss_param();
    params_.l2_per_location = lp.l2_per_location();
    params_.l2_prescale_by_channels = lp.l2_prescale_by_channels();
    params_.normalize_by_num_entries = lp.normalize_by_num_entries();
    params_.epsilon = lp.epsilon();
    params_.plateau = lp.plateau();
  }
  virtual void Reshape(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    top[0]->Reshape(vector<int>());   // Loss layers output a scalar; 0 axes.
    const size_t need = fn2_l1loss_workspace_bytes(bottom[0]->num(), bottom[0]->channels(), bottom[0]->height(), bottom[0]->width());
    workspace_.Reshape(vector<int>{(int)((need + sizeof(Dtype) - 1) / sizeof(Dtype))});
    loss_dev_.Reshape(vector<int>{1});
  }
  virtual inline const char* type() const { return "L1Loss"; }
  virtual inline int ExactNumBottomBlobs() const { return -1; }
  virtual inline int MinBottomBlobs() const { return 1; }
  virtual inline int MaxBottomBlobs() const { return 2; }
  virtual inline int ExactNumTopBlobs() const { return 1; }
  virtual inline bool AllowForceBackward(const int) const { return true; }

 protected:
  virtual void Forward_cpu(const vector<Blob<Dtype>*>&, const vector<Blob<Dtype>*>&) { NOT_IMPLEMENTED; }
  virtual void Backward_cpu(const vector<Blob<Dtype>*>&, const vector<bool>&, const vector<Blob<Dtype>*>&) { NOT_IMPLEMENTED; }
  virtual void Forward_gpu(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    FN2_CALL(fn2_l1loss_forward(&params_, f32(bottom[0]->gpu_data()), bottom.size() > 1 ? f32(bottom[1]->gpu_data()) : nullptr,
                                f32(loss_dev_.mutable_gpu_data()), bottom[0]->num(), bottom[0]->channels(), bottom[0]->height(),
                                bottom[0]->width(), f32(workspace_.mutable_gpu_data()), workspace_.count() * sizeof(Dtype), kStream));
    top[0]->mutable_cpu_data()[0] = loss_dev_.cpu_data()[0];   // the reference also writes the scalar on the host (l1loss_layer.cu:142)
  }
  virtual void Backward_gpu(const vector<Blob<Dtype>*>& top, const vector<bool>& propagate_down, const vector<Blob<Dtype>*>& bottom) {
    bool prop_down = propagate_down[0];
    if (bottom.size() > 1) prop_down |= propagate_down[1];
    if (!prop_down) return;
    FN2_CALL(fn2_l1loss_backward(&params_, f32(bottom[0]->gpu_data()), bottom.size() > 1 ? f32(bottom[1]->gpu_data()) : nullptr,
                                 top[0]->cpu_diff()[0], f32(bottom[0]->mutable_gpu_diff()),
                                 bottom.size() > 1 ? f32(bottom[1]->mutable_gpu_diff()) : nullptr, bottom[0]->num(), bottom[0]->channels(),
                                 bottom[0]->height(), bottom[0]->width(), f32(workspace_.mutable_gpu_data()),
                                 workspace_.count() * sizeof(Dtype), kStream));
  }
  fn2_l1loss_params params_;
  Blob<Dtype> workspace_, loss_dev_;
};

// ---------------------------------------------------------------------------------------------------------
// LpqLoss (include/caffe/layers/lpq_loss_layer.hpp; lpq_loss_layer.cpp:14-173, lpq_loss_layer.cu:97-245) on the fused kernels of
// include/flownet2_hip_lpq_loss.h.  No state between forward and backward but the workspace ({loss, normalize_coeff} stay on the
// device): p and q are picked from the schedule by the net's iteration in both passes -- a pure function of it, where the reference pops a
// queue and never steps back.
template <typename Dtype>
class LpqLossLayer : public Layer<Dtype> {
 public:
  explicit LpqLossLayer(const LayerParameter& param) : Layer<Dtype>(param) {}
  virtual void LayerSetUp(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    if (this->layer_param_.loss_weight_size() == 0) this->layer_param_.add_loss_weight(Dtype(1));   // LossLayer::LayerSetUp, loss_layer.cpp:8-13
    const LpqLossParameter& lp = this->layer_param_.lpq_loss_param();
    const int ns = lp.pq_episode_starts_at_iter_size(), np = lp.p_size(), nq = lp.q_size();
    starts_.clear(); ps_.clear(); qs_.clear();
    if (ns == 0 && np == 1 && nq == 1) {                                                            // lpq_loss_layer.cpp:29-37
      starts_.push_back(0);
    } else {
      if (ns != np || np != nq)                                                                     // cpp:41-47
        LOG(FATAL) << "Incompatible sizes: (pq_episode_starts_at_iter -> " << ns << ", p -> " << np << ", q -> " << nq << ")";
      if (ns < 1) LOG(FATAL) << "Lpq schedule parameters must not be empty";                        // cpp:49-51
      for (int i = 0; i + 1 < ns; ++i)                                                              // cpp:53-64
        if (lp.pq_episode_starts_at_iter(i) >= lp.pq_episode_starts_at_iter(i + 1)) {
          std::ostringstream oss;
          for (int j = 0; j < ns; ++j) oss << " " << lp.pq_episode_starts_at_iter(j);
          LOG(FATAL) << "pq_episode_starts_at_frame is not ordered or contains duplicates:" << oss.str();
        }
      if (lp.pq_episode_starts_at_iter(0) != 0)                                                     // cpp:66-69
        LOG(FATAL) << "First entry in pq_episode_starts_at_frame is not 0, this is probably a mistake.";
      for (int i = 0; i < ns; ++i) starts_.push_back((int)lp.pq_episode_starts_at_iter(i));
    }
    for (int i = 0; i < np; ++i) { ps_.push_back(lp.p(i)); qs_.push_back(lp.q(i)); }
    if (bottom.size() != 1 && bottom.size() != 2) LOG(FATAL) << "LpqLossLayer needs one or two input blobs.";   // cpp:98-100
  }
  virtual void Reshape(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    top[0]->Reshape(vector<int>());   // Loss layers output a scalar; 0 axes.
    size_t need = 0;
    FN2_CALL(fn2_lpq_loss_sizes(1, &need, nullptr, nullptr));
    workspace_.Reshape(vector<int>{(int)((need + sizeof(Dtype) - 1) / sizeof(Dtype))});
    loss_dev_.Reshape(vector<int>{1});
  }
  virtual inline const char* type() const { return "LpqLoss"; }
  virtual inline int ExactNumBottomBlobs() const { return -1; }
  virtual inline int MinBottomBlobs() const { return 1; }
  virtual inline int MaxBottomBlobs() const { return 2; }
  virtual inline int ExactNumTopBlobs() const { return 1; }
  virtual inline bool AutoTopBlobs() const { return true; }
  virtual inline bool AllowForceBackward(const int) const { return true; }

 protected:
  // the episode in force at the net's iteration (lpq_loss_layer.cu:100-135; 0 without a net)
  int Episode() {
    Net<Dtype>* net = this->GetNet();
    const int step = fn2_lpq_loss_schedule_step((int)starts_.size(), starts_.data(), net ? net->iter() : 0);
    return step < 0 ? 0 : step;
  }
  virtual void Forward_cpu(const vector<Blob<Dtype>*>&, const vector<Blob<Dtype>*>&) { NOT_IMPLEMENTED; }
  virtual void Backward_cpu(const vector<Blob<Dtype>*>&, const vector<bool>&, const vector<Blob<Dtype>*>&) { NOT_IMPLEMENTED; }
  virtual void Forward_gpu(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    const LpqLossParameter& lp = this->layer_param_.lpq_loss_param();
    const int e = Episode();
    FN2_CALL(fn2_lpq_loss_forward(f32(bottom[0]->gpu_data()), bottom.size() > 1 ? f32(bottom[1]->gpu_data()) : nullptr,
                                  f32(loss_dev_.mutable_gpu_data()), bottom[0]->num(), bottom[0]->channels(), bottom[0]->height(),
                                  bottom[0]->width(), ps_[e], qs_[e], lp.p_epsilon(), lp.q_epsilon(), lp.l2_prescale_by_channels(),
                                  lp.normalize_by_num_entries(), f32(workspace_.mutable_gpu_data()), workspace_.count() * sizeof(Dtype), kStream));
    top[0]->mutable_cpu_data()[0] = loss_dev_.cpu_data()[0];   // the reference also writes the scalar on the host (lpq_loss_layer.cu:197)
  }
  virtual void Backward_gpu(const vector<Blob<Dtype>*>& top, const vector<bool>& propagate_down, const vector<Blob<Dtype>*>& bottom) {
    bool prop_down = propagate_down[0];
    if (bottom.size() > 1) prop_down |= propagate_down[1];
    if (!prop_down) return;
    const LpqLossParameter& lp = this->layer_param_.lpq_loss_param();
    const int e = Episode();
    FN2_CALL(fn2_lpq_loss_backward(f32(bottom[0]->gpu_data()), bottom.size() > 1 ? f32(bottom[1]->gpu_data()) : nullptr,
                                   top[0]->cpu_diff()[0], f32(bottom[0]->mutable_gpu_diff()),
                                   bottom.size() > 1 ? f32(bottom[1]->mutable_gpu_diff()) : nullptr, bottom[0]->num(), bottom[0]->channels(),
                                   bottom[0]->height(), bottom[0]->width(), ps_[e], qs_[e], lp.p_epsilon(), lp.q_epsilon(),
                                   lp.l2_prescale_by_channels(), lp.normalize_by_num_entries(), f32(workspace_.mutable_gpu_data()),
                                   workspace_.count() * sizeof(Dtype), kStream));
  }
  vector<int> starts_;
  vector<float> ps_, qs_;
  Blob<Dtype> workspace_, loss_dev_;
};

// ---------------------------------------------------------------------------------------------------------
template <typename Dtype>
class ChannelNormLayer : public Layer<Dtype> {
 public:
  explicit ChannelNormLayer(const LayerParameter& param) : Layer<Dtype>(param) {}
  virtual void Reshape(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    CHECK_EQ(bottom.size(), 1u) << "ChannelNormLayer takes two input blobs: image and flow.";   // (sic) channel_norm_layer.cpp:30
    CHECK_EQ(top.size(), 1u) << "ChannelNormLayer outputs one blob.";
    top[0]->Reshape(bottom[0]->num(), 1, bottom[0]->height(), bottom[0]->width());
  }
  virtual inline const char* type() const { return "NormLayer"; }   // (sic) channel_norm_layer.hpp:22
  virtual inline int MinBottomBlobs() const { return 1; }
  virtual inline int ExactNumTopBlobs() const { return 1; }

 protected:
  virtual void Forward_cpu(const vector<Blob<Dtype>*>&, const vector<Blob<Dtype>*>&) { NOT_IMPLEMENTED; }
  virtual void Backward_cpu(const vector<Blob<Dtype>*>&, const vector<bool>&, const vector<Blob<Dtype>*>&) { NOT_IMPLEMENTED; }
  virtual void Forward_gpu(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    FN2_CALL(fn2_channel_norm_forward(f32(bottom[0]->gpu_data()), f32(top[0]->mutable_gpu_data()), bottom[0]->num(), bottom[0]->channels(),
                                      bottom[0]->height(), bottom[0]->width(), kStream));
  }
  virtual void Backward_gpu(const vector<Blob<Dtype>*>& top, const vector<bool>&, const vector<Blob<Dtype>*>& bottom) {
    FN2_CALL(fn2_channel_norm_backward(f32(bottom[0]->gpu_data()), f32(top[0]->gpu_data()), f32(top[0]->gpu_diff()), f32(bottom[0]->mutable_gpu_diff()),
                                       bottom[0]->num(), bottom[0]->channels(), bottom[0]->height(), bottom[0]->width(), kStream));
  }
};

// ---------------------------------------------------------------------------------------------------------
template <typename Dtype>
class DownsampleLayer : public Layer<Dtype> {
 public:
  explicit DownsampleLayer(const LayerParameter& param) : Layer<Dtype>(param) {}
  virtual void Reshape(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    this->layer_param_.set_reshape_every_iter(false);
    LOG(WARNING) << "DownsampleLayer only runs Reshape on setup";
    CHECK_GE(bottom.size(), 1u);
    CHECK_LE(bottom.size(), 2u);
    CHECK_EQ(top.size(), 1u);
    if (bottom.size() == 1) {
      top_height_ = this->layer_param_.downsample_param().top_height();
      top_width_ = this->layer_param_.downsample_param().top_width();
    } else {
      top_height_ = bottom[1]->height();
      top_width_ = bottom[1]->width();
    }
    CHECK_GE(top_height_, 1) << "DownsampleLayer must have top_height > 0";
    CHECK_GE(top_width_, 1) << "DownsampleLayer must have top_width > 0";
    top[0]->Reshape(bottom[0]->num(), bottom[0]->channels(), top_height_, top_width_);
    // the reference shares data/diff with the bottom when the sizes agree (downsample_layer.cpp:53-56); we copy in Forward
  }
  virtual inline const char* type() const { return "Downsample"; }
  virtual inline int MinBottomBlobs() const { return 1; }
  virtual inline int MaxBottomBlobs() const { return 2; }
  virtual inline int ExactNumTopBlobs() const { return 1; }
  virtual inline bool AllowBackward() const { return false; }

 protected:
  virtual void Forward_cpu(const vector<Blob<Dtype>*>&, const vector<Blob<Dtype>*>&) { LOG(FATAL) << "DownsampleLayer: CPU Forward not yet implemented."; }
  virtual void Backward_cpu(const vector<Blob<Dtype>*>&, const vector<bool>&, const vector<Blob<Dtype>*>&) { LOG(FATAL) << "DownsampleLayer cannot do backward."; }
  virtual void Forward_gpu(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    FN2_CALL(fn2_downsample_forward(f32(bottom[0]->gpu_data()), f32(top[0]->mutable_gpu_data()), bottom[0]->num(), bottom[0]->channels(),
                                    bottom[0]->height(), bottom[0]->width(), top_height_, top_width_, kStream));
  }
  virtual void Backward_gpu(const vector<Blob<Dtype>*>&, const vector<bool>& propagate_down, const vector<Blob<Dtype>*>&) {
    for (size_t i = 0; i < propagate_down.size(); i++)
      if (propagate_down[i]) LOG(FATAL) << "DownsamplingLayer cannot do backward.";
  }
  int top_width_, top_height_;
};

// ---------------------------------------------------------------------------------------------------------
// Convolution / Deconvolution as plug-ins: one class for both (transposed_ tells them apart), the kernel family picked by the LIBRARY from
// the layer's geometry (fn2_conv_route / fn2_deconv_route, csrc/conv_route.cpp -- the routing the benchmarks ran with).
//   <- ConvolutionLayer / DeconvolutionLayer (conv_layer.cpp:8-40, deconv_layer.cpp:8-45) over BaseConvolutionLayer::LayerSetUp / Reshape
//      (base_conv_layer.cpp:14-253): same convolution_param fields (num_output, kernel_size, stride, pad, bias_term, weight / bias fillers),
//      same blob shapes -- weight [num_output, C, k, k] (Deconvolution: [C, num_output, k, k]), bias [num_output] --, same top shape.
// Scope: every ConvolutionParameter the stock layers accept over 0 to 3 spatial axes -- axis (the axes in front of it fold into the batch,
// base_conv_layer.cpp:17-21, 191), kernel_size, stride, pad, dilation once or once per spatial axis, kernel_h / kernel_w and their kin with two
// spatial axes, group, force_nd_im2col (it chooses an im2col routine in the reference and nothing here) -- read with the checks and messages
// of base_conv_layer.cpp:24-124; one bottom / top pair.  Refused, with a message naming the layer and the count: four or more spatial axes.
// A PLAIN layer (two spatial axes, square taps, one stride, one pad, dilation 1, group 1) takes the path it always took: every Convolution and Deconvolution of the FlowNet graphs runs on its specialised family; a
// geometry no family takes -- and a gradient pass of a layer whose forward has a family but that pass none -- runs on the general kernels
// (csrc/conv_general.hip).  Every other layer runs forward and all three gradient passes on the same kernels.  Both reach them through
// the 19 ints of include/flownet2_hip_conv_volume.h (fewer than three spatial axes with the leading ones trivial: the kernels and the bits of
// include/flownet2_hip_conv_general.h for a plain layer, of include/flownet2_hip_conv_geometry.h for the others).  Only what
// fn2_conv_volume_supported refuses (an empty output, a blob beyond the 32-bit index limits) aborts in Reshape with a message naming the layer.
// The packed weight operand (round 6): packed ONCE and kept while the weights provably have not changed -- Caffe has no "weights changed"
// signal below Solver::ApplyUpdate, so the layer reads what SyncedMemory already records: the operand is reused iff the layer runs in the
// TEST phase, the weight blob's memory is SYNCED on entry (no mutable_cpu_data / mutable_gpu_data since the last const access: a
// CopyTrainedLayersFrom, a pycaffe `net.params[...]` write or a device-side update all leave HEAD_AT_CPU / HEAD_AT_GPU), its SyncedMemory is
// not shared with another blob (a solver's test net shares the train net's weights, Net::ShareTrainedLayersWith: those are updated behind
// this layer's back and re-synced by snapshots), and the device pointer is the one that was packed.  Everything else -- every TRAIN-phase
// forward -- repacks.  fn2_caffe_adapter_stats() counts packs and reuses (tests/test_caffe_adapter.py).
// Backward_gpu (conv_layer.cu:26-60 / deconv_layer.cu:27-58) runs the library's own gradient routes; parameter diffs are accumulated.
struct Fn2AdapterStats { long long weight_packs, weight_pack_reuses; };
inline Fn2AdapterStats& fn2_adapter_stats() { static Fn2AdapterStats s{0, 0}; return s; }

template <typename Dtype>
class Fn2ConvolutionLayer : public Layer<Dtype> {
 public:
  explicit Fn2ConvolutionLayer(const LayerParameter& param, bool transposed) : Layer<Dtype>(param), transposed_(transposed) {}
  virtual void LayerSetUp(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    const ConvolutionParameter& cp = this->layer_param_.convolution_param();
    // base_conv_layer.cpp:14-124, with its messages
    channel_axis_ = bottom[0]->CanonicalAxisIndex(cp.axis());
    num_spatial_axes_ = bottom[0]->num_axes() - channel_axis_ - 1;
    CHECK_GE(num_spatial_axes_, 0);
    CHECK_LE(num_spatial_axes_, 3) << this->layer_param_.name() << ": libflownet2_hip runs convolutions over 0 to 3 spatial axes; "
                                   << num_spatial_axes_ << " were asked for";
    const int num_spatial_axes = num_spatial_axes_, lead = 3 - num_spatial_axes;
    // the values per axis (depth, height, width); the axes that are not there are trivial: kernel 1, stride 1, pad 0, dilation 1
    for (int i = 0; i < 3; ++i) { kernel_3_[i] = 1; stride_3_[i] = 1; pad_3_[i] = 0; dilation_3_[i] = 1; }
    if (cp.has_kernel_h() || cp.has_kernel_w()) {
      CHECK_EQ(num_spatial_axes, 2) << "kernel_h & kernel_w can only be used for 2D convolution.";
      CHECK_EQ(0, cp.kernel_size_size()) << "Either kernel_size or kernel_h/w should be specified; not both.";
      kernel_3_[1] = (int)cp.kernel_h(); kernel_3_[2] = (int)cp.kernel_w();
    } else {
      const int n = cp.kernel_size_size();
      CHECK(n == 1 || n == num_spatial_axes) << "kernel_size must be specified once, or once per spatial dimension "
                                             << "(kernel_size specified " << n << " times; " << num_spatial_axes << " spatial dims).";
      for (int i = 0; i < num_spatial_axes; ++i) kernel_3_[lead + i] = (int)cp.kernel_size(n == 1 ? 0 : i);
    }
    for (int i = 0; i < 3; ++i) CHECK_GT(kernel_3_[i], 0) << "Filter dimensions must be nonzero.";
    if (cp.has_stride_h() || cp.has_stride_w()) {
      CHECK_EQ(num_spatial_axes, 2) << "stride_h & stride_w can only be used for 2D convolution.";
      CHECK_EQ(0, cp.stride_size()) << "Either stride or stride_h/w should be specified; not both.";
      stride_3_[1] = (int)cp.stride_h(); stride_3_[2] = (int)cp.stride_w();
    } else {
      const int n = cp.stride_size();
      CHECK(n == 0 || n == 1 || n == num_spatial_axes) << "stride must be specified once, or once per spatial dimension "
                                                       << "(stride specified " << n << " times; " << num_spatial_axes << " spatial dims).";
      for (int i = 0; i < num_spatial_axes && n; ++i) stride_3_[lead + i] = (int)cp.stride(n == 1 ? 0 : i);
    }
    for (int i = 0; i < 3; ++i) CHECK_GT(stride_3_[i], 0) << "Stride dimensions must be nonzero.";
    if (cp.has_pad_h() || cp.has_pad_w()) {
      CHECK_EQ(num_spatial_axes, 2) << "pad_h & pad_w can only be used for 2D convolution.";
      CHECK_EQ(0, cp.pad_size()) << "Either pad or pad_h/w should be specified; not both.";
      pad_3_[1] = (int)cp.pad_h(); pad_3_[2] = (int)cp.pad_w();
    } else {
      const int n = cp.pad_size();
      CHECK(n == 0 || n == 1 || n == num_spatial_axes) << "pad must be specified once, or once per spatial dimension "
                                                       << "(pad specified " << n << " times; " << num_spatial_axes << " spatial dims).";
      for (int i = 0; i < num_spatial_axes && n; ++i) pad_3_[lead + i] = (int)cp.pad(n == 1 ? 0 : i);
    }
    {
      const int n = cp.dilation_size();
      CHECK(n == 0 || n == 1 || n == num_spatial_axes) << "dilation must be specified once, or once per spatial dimension "
                                                       << "(dilation specified " << n << " times; " << num_spatial_axes << " spatial dims).";
      for (int i = 0; i < num_spatial_axes && n; ++i) dilation_3_[lead + i] = (int)cp.dilation(n == 1 ? 0 : i);
    }
    for (int i = 0; i < 3; ++i) CHECK_GT(dilation_3_[i], 0) << "Dilation dimensions must be nonzero.";
    kernel_h_ = kernel_3_[1]; kernel_w_ = kernel_3_[2]; stride_h_ = stride_3_[1]; stride_w_ = stride_3_[2]; pad_h_ = pad_3_[1]; pad_w_ = pad_3_[2];
    dilation_h_ = dilation_3_[1]; dilation_w_ = dilation_3_[2];
    num_output_ = (int)cp.num_output();
    CHECK_GT(num_output_, 0);
    bias_term_ = cp.bias_term();
    channels_ = bottom[0]->shape(channel_axis_);
    group_ = (int)cp.group();
    CHECK_GT(group_, 0);
    CHECK_EQ(channels_ % group_, 0);
    CHECK_EQ(num_output_ % group_, 0) << "Number of output should be multiples of group.";
    // a PLAIN layer (all a FlowNet has) keeps the specialised route and the square-tap general kernels behind it
    plain_ = num_spatial_axes == 2 && kernel_h_ == kernel_w_ && stride_h_ == stride_w_ && pad_h_ == pad_w_ && dilation_h_ == 1 && dilation_w_ == 1 &&
             group_ == 1;
    kernel_ = kernel_h_; stride_ = stride_h_; pad_ = pad_h_;      // read by the plain paths only
    if (this->blobs_.size() == 0) {
      this->blobs_.resize(bias_term_ ? 2 : 1);
      // base_conv_layer.cpp:125-139: [conv_out_channels, conv_in_channels / group, k...]; for a Deconvolution the roles are swapped
      vector<int> wshape{transposed_ ? channels_ : num_output_, (transposed_ ? num_output_ : channels_) / group_};
      for (int i = 0; i < num_spatial_axes; ++i) wshape.push_back(kernel_3_[lead + i]);
      this->blobs_[0].reset(new Blob<Dtype>(wshape));
      shared_ptr<Filler<Dtype> > wf(GetFiller<Dtype>(cp.weight_filler()));
      wf->Fill(this->blobs_[0].get());
      if (bias_term_) {
        this->blobs_[1].reset(new Blob<Dtype>(vector<int>{num_output_}));
        shared_ptr<Filler<Dtype> > bf(GetFiller<Dtype>(cp.bias_filler()));
        bf->Fill(this->blobs_[1].get());
      }
    }
    this->param_propagate_down_.resize(this->blobs_.size(), true);
  }
  virtual void Reshape(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    CHECK_EQ(bottom[0]->num_axes(), channel_axis_ + 1 + num_spatial_axes_) << "bottom num_axes may not change.";
    CHECK_EQ(bottom[0]->shape(channel_axis_), channels_) << "Input size incompatible with convolution kernel.";
    // every axis in front of the channels folds into the batch (base_conv_layer.cpp:191); the spatial extents right-aligned in (D, H, W)
    for (int i = 0; i < 3; ++i) in_3_[i] = 1;
    for (int i = 0; i < num_spatial_axes_; ++i) in_3_[3 - num_spatial_axes_ + i] = bottom[0]->shape(channel_axis_ + 1 + i);
    desc_.N = bottom[0]->count(0, channel_axis_); desc_.Cin = channels_; desc_.Hin = in_3_[1]; desc_.Win = in_3_[2];
    desc_.Cout = num_output_; desc_.kernel = kernel_; desc_.stride = stride_; desc_.pad = pad_;
    const int tr = transposed_ ? 1 : 0;
    // what the general kernels are called with, for every layer (a plain one: depth trivial, dilation 1, group 1)
    const int g[19] = {desc_.N, channels_, in_3_[0], in_3_[1], in_3_[2], num_output_, kernel_3_[0], kernel_3_[1], kernel_3_[2], stride_3_[0], stride_3_[1],
                       stride_3_[2], pad_3_[0], pad_3_[1], pad_3_[2], dilation_3_[0], dilation_3_[1], dilation_3_[2], group_};
    std::copy(g, g + 19, geom_);
    general_ = fn2_conv_volume_supported(geom_, tr) != 0;
    size_t gen_fwd = 0, gen_dgrad = 0, gen_ws = 0;
    if (general_) FN2_CALL(fn2_conv_volume_sizes(geom_, tr, &gen_fwd, &gen_dgrad, nullptr, &gen_ws));
    if (!plain_) { ReshapeGeometry(bottom, top, gen_fwd, gen_dgrad, gen_ws); return; }
    int oh, ow;
    if (transposed_) {      // deconv_layer.cpp:8-24
      oh = stride_ * (desc_.Hin - 1) + kernel_ - 2 * pad_; ow = stride_ * (desc_.Win - 1) + kernel_ - 2 * pad_;
      route_ = fn2_deconv_route(&desc_, 0);
    } else {                // conv_layer.cpp:8-23
      oh = (desc_.Hin + 2 * pad_ - kernel_) / stride_ + 1; ow = (desc_.Win + 2 * pad_ - kernel_) / stride_ + 1;
      route_ = fn2_conv_route(&desc_, 0);
    }
    // the general kernels: the forward of a geometry no family takes, and below the gradient passes that have no route of their own
    if (route_ == 0 && !general_)
      LOG(FATAL) << this->layer_param_.name() << ": libflownet2_hip has no kernel for " << type() << "{kernel " << kernel_ << ", stride " << stride_
                 << ", pad " << pad_ << "} " << channels_ << " -> " << num_output_ << " on " << desc_.Hin << " x " << desc_.Win
                 << " (empty output, or a blob beyond the 32-bit index limits)";
    out_h_ = oh; out_w_ = ow;
    top[0]->Reshape(TopShape(bottom, 1, oh, ow));
    const size_t pf = route_ == 0 ? gen_fwd : transposed_ ? fn2_deconv_packed_weight_floats(&desc_, route_) : fn2_conv_packed_weight_floats(&desc_, route_);
    size_t wb = route_ == 0 ? 0 : transposed_ ? fn2_deconv_workspace_bytes(&desc_, route_) : fn2_conv_workspace_bytes(&desc_, route_);
    packed_.Reshape(vector<int>{(int)pf});
    // backward: the library's own routes (csrc/conv_route.cpp); one scratch blob serves every call of the layer (they run in stream order)
    bwd_route_ = fn2_conv_backward_data_route(&desc_, transposed_);
    bwd_weights_ = fn2_conv_backward_weights_supported(&desc_, transposed_) != 0;
    wb = std::max(wb, fn2_bias_leaky_relu_backward_workspace_bytes(desc_.N, num_output_, oh, ow));
    head_ = transposed_ ? route_ == FN2_DECONV_ROUTE_HEAD : route_ == FN2_CONV_ROUTE_HEAD;      // the 2-channel flow heads: kernels of their own, forward and backward
    if (head_) wb = std::max(wb, transposed_ ? fn2_upsample_flow_deconv_backward_workspace_bytes(desc_.N, desc_.Hin, desc_.Win)
                                             : fn2_predict_flow_conv_backward_workspace_bytes(desc_.N, channels_, desc_.Hin, desc_.Win));
    wb = std::max(wb, fn2_conv_backward_weights_workspace_bytes(&desc_, tr));
    if (!bwd_weights_ && general_ && !head_) wb = std::max(wb, gen_ws);
    if (bwd_route_ == FN2_BWD_ROUTE_NONE && general_ && !head_) packed_bwd_.Reshape(vector<int>{(int)gen_dgrad});
    if (bwd_route_ != FN2_BWD_ROUTE_NONE) {
      wb = std::max(wb, fn2_conv_backward_data_workspace_bytes(&desc_, tr, bwd_route_));
      wb = std::max(wb, fn2_conv_backward_data_pack_workspace_bytes(&desc_, tr, bwd_route_));
      packed_bwd_.Reshape(vector<int>{(int)fn2_conv_backward_data_packed_weight_floats(&desc_, tr, bwd_route_)});
    }
    workspace_.Reshape(vector<int>{(int)((wb + 3) / 4) + 4});
  }
  // the top shape: the bottom's leading axes, num_output, the output extents of the spatial axes the layer has (base_conv_layer.cpp:198-207)
  vector<int> TopShape(const vector<Blob<Dtype>*>& bottom, int od, int oh, int ow) const {
    vector<int> shape(bottom[0]->shape().begin(), bottom[0]->shape().begin() + channel_axis_);
    shape.push_back(num_output_);
    const int out[3] = {od, oh, ow};
    for (int i = 3 - num_spatial_axes_; i < 3; ++i) shape.push_back(out[i]);
    return shape;
  }
  // a layer that is not plain: no specialised route, all four passes on the general kernels
  void ReshapeGeometry(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top, size_t gen_fwd, size_t gen_dgrad, size_t gen_ws) {
    route_ = 0; bwd_route_ = FN2_BWD_ROUTE_NONE; bwd_weights_ = false; head_ = false;
    if (!general_ && num_spatial_axes_ == 3)
      LOG(FATAL) << this->layer_param_.name() << ": libflownet2_hip has no kernel for " << type() << "{kernel " << kernel_3_[0] << " x " << kernel_h_ << " x "
                 << kernel_w_ << ", stride " << stride_3_[0] << " x " << stride_h_ << " x " << stride_w_ << ", pad " << pad_3_[0] << " x " << pad_h_ << " x "
                 << pad_w_ << ", dilation " << dilation_3_[0] << " x " << dilation_h_ << " x " << dilation_w_ << ", group " << group_ << "} " << channels_
                 << " -> " << num_output_ << " on " << in_3_[0] << " x " << desc_.Hin << " x " << desc_.Win
                 << " (empty output, or a blob beyond the 32-bit index limits)";
    if (!general_)
      LOG(FATAL) << this->layer_param_.name() << ": libflownet2_hip has no kernel for " << type() << "{kernel " << kernel_h_ << " x " << kernel_w_
                 << ", stride " << stride_h_ << " x " << stride_w_ << ", pad " << pad_h_ << " x " << pad_w_ << ", dilation " << dilation_h_ << " x "
                 << dilation_w_ << ", group " << group_ << "} " << channels_ << " -> " << num_output_ << " on " << desc_.Hin << " x " << desc_.Win
                 << " (empty output, or a blob beyond the 32-bit index limits)";
    int od = 0, oh = 0, ow = 0;
    FN2_CALL(fn2_conv_volume_out_shape(geom_, transposed_ ? 1 : 0, &od, &oh, &ow));      // conv_layer.cpp:8-23 / deconv_layer.cpp:8-24 with the dilated extent
    out_h_ = od * oh; out_w_ = ow;      // what the bias gradient sums over, per channel
    top[0]->Reshape(TopShape(bottom, od, oh, ow));
    packed_.Reshape(vector<int>{(int)gen_fwd});
    packed_bwd_.Reshape(vector<int>{(int)gen_dgrad});
    const size_t wb = std::max(gen_ws, fn2_bias_leaky_relu_backward_workspace_bytes(desc_.N, num_output_, out_h_, out_w_));
    workspace_.Reshape(vector<int>{(int)((wb + 3) / 4) + 4});
  }
  virtual inline const char* type() const { return transposed_ ? "Deconvolution" : "Convolution"; }
  virtual inline int ExactNumBottomBlobs() const { return 1; }
  virtual inline int ExactNumTopBlobs() const { return 1; }

 protected:
  virtual void Forward_cpu(const vector<Blob<Dtype>*>&, const vector<Blob<Dtype>*>&) { NOT_IMPLEMENTED; }
  virtual void Backward_cpu(const vector<Blob<Dtype>*>&, const vector<bool>&, const vector<Blob<Dtype>*>&) { NOT_IMPLEMENTED; }
  virtual void Forward_gpu(const vector<Blob<Dtype>*>& bottom, const vector<Blob<Dtype>*>& top) {
    // decided BEFORE gpu_data() touches the head state (see the class comment)
    const bool untouched = this->blobs_[0]->data()->head() == SyncedMemory::SYNCED && this->blobs_[0]->data().use_count() == 1;
    const float* w = f32(this->blobs_[0]->gpu_data());
    const float* b = bias_term_ ? f32(this->blobs_[1]->gpu_data()) : nullptr;
    const bool reuse = this->phase_ == TEST && untouched && packed_for_ == w && packed_route_ == route_ && packed_count_ == packed_.count();
    float* pk = f32(packed_.mutable_gpu_data());
    void* ws = workspace_.mutable_gpu_data();
    const size_t wsb = sizeof(Dtype) * (size_t)workspace_.count();
    if (reuse) {
      fn2_adapter_stats().weight_pack_reuses++;
    } else {
      if (route_ == 0) FN2_CALL(fn2_conv_volume_pack_weights(geom_, transposed_ ? 1 : 0, 0, w, pk, kStream));
      else if (transposed_) FN2_CALL(fn2_deconv_pack_weights(&desc_, route_, w, pk, kStream));
      else FN2_CALL(fn2_conv_pack_weights(&desc_, route_, w, pk, kStream));
      packed_for_ = w; packed_route_ = route_; packed_count_ = packed_.count();
      fn2_adapter_stats().weight_packs++;
    }
    if (route_ == 0) {
      FN2_CALL(fn2_conv_volume_forward(geom_, transposed_ ? 1 : 0, f32(bottom[0]->gpu_data()), channels_, 0, pk, b, f32(top[0]->mutable_gpu_data()),
                                       num_output_, 0, 0, 0.f, kStream));
    } else if (transposed_) {
      FN2_CALL(fn2_deconv_forward(&desc_, route_, f32(bottom[0]->gpu_data()), channels_, 0, pk, b, f32(top[0]->mutable_gpu_data()), num_output_, 0,
                                  0, 0.f, ws, wsb, kStream));
    } else {
      FN2_CALL(fn2_conv_forward(&desc_, route_, f32(bottom[0]->gpu_data()), channels_, 0, pk, b, f32(top[0]->mutable_gpu_data()), num_output_, 0,
                                0, 0.f, ws, wsb, kStream));
    }
  }
  // conv_layer.cu:26-60 / deconv_layer.cu:27-58: bias_diff += sum of top_diff (backward_gpu_bias), weight_diff += ... (weight_gpu_gemm, beta = 1:
  // the solver clears the parameter diffs once per iteration), bottom_diff = ... (backward_gpu_gemm / forward_gpu_gemm: overwritten)
  virtual void Backward_gpu(const vector<Blob<Dtype>*>& top, const vector<bool>& propagate_down, const vector<Blob<Dtype>*>& bottom) {
    const int tr = transposed_ ? 1 : 0;
    const float* td = f32(top[0]->gpu_diff());
    void* ws = workspace_.mutable_gpu_data();
    const size_t wsb = sizeof(Dtype) * (size_t)workspace_.count();
    if (head_) {
      // predict_flow* / upsample_flow*: one call computes the three gradients (csrc/flow_head_bwd.hip); parameter diffs accumulate, NULL = not wanted
      float* bd = propagate_down[0] ? f32(bottom[0]->mutable_gpu_diff()) : nullptr;
      float* wd = this->param_propagate_down_[0] ? f32(this->blobs_[0]->mutable_gpu_diff()) : nullptr;
      float* db = (bias_term_ && this->param_propagate_down_[1]) ? f32(this->blobs_[1]->mutable_gpu_diff()) : nullptr;
      const float* w = f32(this->blobs_[0]->gpu_data());
      if (transposed_) {
        FN2_CALL(fn2_upsample_flow_deconv_backward(f32(bottom[0]->gpu_data()), w, td, bd, wd, db, desc_.N, desc_.Hin, desc_.Win, 1, ws, wsb, kStream));
      } else {
        if (!fn2_predict_flow_conv_backward_supported(desc_.N, channels_, desc_.Hin, desc_.Win))
          LOG(FATAL) << this->layer_param_.name() << ": libflownet2_hip has no backward kernel for this flow head; keep the stock layer for it";
        FN2_CALL(fn2_predict_flow_conv_backward(f32(bottom[0]->gpu_data()), channels_, 0, w, td, bd, wd, db, desc_.N, channels_, desc_.Hin, desc_.Win, 1, ws, wsb, kStream));
      }
      return;
    }
    if (bias_term_ && this->param_propagate_down_[1])
      FN2_CALL(fn2_conv_backward_bias(td, num_output_, 0, f32(this->blobs_[1]->mutable_gpu_diff()), desc_.N, num_output_, out_h_, out_w_,
                                      1, ws, wsb, kStream));
    if (this->param_propagate_down_[0]) {
      if (!bwd_weights_ && !general_)
        LOG(FATAL) << this->layer_param_.name() << ": libflownet2_hip has no weight-gradient kernel for this " << type();
      if (bwd_weights_) {
        FN2_CALL(fn2_conv_backward_weights(&desc_, tr, f32(bottom[0]->gpu_data()), channels_, 0, td, num_output_, 0, f32(this->blobs_[0]->mutable_gpu_diff()),
                                           1, ws, wsb, kStream));
      } else {      // the general kernel (the bias gradient was taken above)
        FN2_CALL(fn2_conv_volume_backward_weights(geom_, tr, f32(bottom[0]->gpu_data()), channels_, 0, td, num_output_, 0,
                                                  f32(this->blobs_[0]->mutable_gpu_diff()), nullptr, 1, ws, wsb, kStream));
      }
    }
    if (propagate_down[0]) {
      if (bwd_route_ == FN2_BWD_ROUTE_NONE && !general_)
        LOG(FATAL) << this->layer_param_.name() << ": libflownet2_hip has no data-gradient kernel for this " << type();
      float* pk = f32(packed_bwd_.mutable_gpu_data());
      if (bwd_route_ == FN2_BWD_ROUTE_NONE) {
        FN2_CALL(fn2_conv_volume_pack_weights(geom_, tr, 1, f32(this->blobs_[0]->gpu_data()), pk, kStream));
        FN2_CALL(fn2_conv_volume_backward_data(geom_, tr, td, num_output_, 0, pk, f32(bottom[0]->mutable_gpu_diff()), channels_, 0, kStream));
        return;
      }
      FN2_CALL(fn2_conv_backward_data_pack_weights(&desc_, tr, bwd_route_, f32(this->blobs_[0]->gpu_data()), pk, ws, wsb, kStream));
      // bottom_room = channels_: a Caffe blob has no room for the channel groups the kernels round up to (the result goes through the scratch)
      FN2_CALL(fn2_conv_backward_data(&desc_, tr, bwd_route_, td, num_output_, 0, pk, f32(bottom[0]->mutable_gpu_diff()), channels_, 0, channels_, ws, wsb, kStream));
    }
  }
  bool transposed_, bias_term_ = true, bwd_weights_ = false, head_ = false, general_ = false, plain_ = true;
  int kernel_ = 0, stride_ = 1, pad_ = 0, num_output_ = 0, channels_ = 0, route_ = 0, bwd_route_ = 0;
  int kernel_h_ = 0, kernel_w_ = 0, stride_h_ = 1, stride_w_ = 1, pad_h_ = 0, pad_w_ = 0, dilation_h_ = 1, dilation_w_ = 1, group_ = 1;
  int channel_axis_ = 1, num_spatial_axes_ = 2, out_h_ = 0, out_w_ = 0;
  int in_3_[3] = {1, 1, 1}, kernel_3_[3] = {1, 1, 1}, stride_3_[3] = {1, 1, 1}, pad_3_[3] = {0, 0, 0}, dilation_3_[3] = {1, 1, 1};      // (depth, height, width)
  fn2_conv_desc desc_;
  int geom_[19] = {0};
  Blob<Dtype> packed_, packed_bwd_, workspace_;
  const float* packed_for_ = nullptr;      // device pointer of the weights packed_ was built from
  int packed_route_ = -1, packed_count_ = -1;
};
template <typename Dtype> shared_ptr<Layer<Dtype> > Creator_Fn2Convolution(const LayerParameter& p) { return shared_ptr<Layer<Dtype> >(new Fn2ConvolutionLayer<Dtype>(p, false)); }
template <typename Dtype> shared_ptr<Layer<Dtype> > Creator_Fn2Deconvolution(const LayerParameter& p) { return shared_ptr<Layer<Dtype> >(new Fn2ConvolutionLayer<Dtype>(p, true)); }

INSTANTIATE_CLASS(CorrelationLayer);
REGISTER_LAYER_CLASS(Correlation);
INSTANTIATE_CLASS(Correlation1DLayer);
REGISTER_LAYER_CLASS(Correlation1D);
INSTANTIATE_CLASS(FlowAugmentationLayer);
REGISTER_LAYER_CLASS(FlowAugmentation);
INSTANTIATE_CLASS(FlowWarpLayer);
REGISTER_LAYER_CLASS(FlowWarp);
INSTANTIATE_CLASS(ResampleLayer);
REGISTER_LAYER_CLASS(Resample);
INSTANTIATE_CLASS(L1LossLayer);
REGISTER_LAYER_CLASS(L1Loss);
INSTANTIATE_CLASS(LpqLossLayer);
REGISTER_LAYER_CLASS(LpqLoss);
INSTANTIATE_CLASS(ChannelNormLayer);
REGISTER_LAYER_CLASS(ChannelNorm);
INSTANTIATE_CLASS(DownsampleLayer);
REGISTER_LAYER_CLASS(Downsample);
// one type string can be registered once (layer_factory.hpp:69-70): in a Caffe tree these two REPLACE GetConvolutionLayer /
// REGISTER_LAYER_CLASS(Deconvolution) of layer_factory.cpp:38-70 / deconv_layer.cpp:79-80 (or wrap them: INTEGRATION.md)
INSTANTIATE_CLASS(Fn2ConvolutionLayer);
REGISTER_LAYER_CREATOR(Convolution, Creator_Fn2Convolution);
REGISTER_LAYER_CREATOR(Deconvolution, Creator_Fn2Deconvolution);

}  // namespace caffe

// weight operands packed / reused by the Convolution and Deconvolution plug-ins of this process (the cache of Fn2ConvolutionLayer)
extern "C" __attribute__((visibility("default"))) long long fn2_caffe_adapter_weight_packs() { return caffe::fn2_adapter_stats().weight_packs; }
extern "C" __attribute__((visibility("default"))) long long fn2_caffe_adapter_weight_pack_reuses() { return caffe::fn2_adapter_stats().weight_pack_reuses; }
