// Stand-in for include/caffe/net.hpp: what a layer with a schedule asks its net (net.hpp:230-231, set by Solver::Step, solver.cpp:202).
#pragma once
#include "caffe/layer.hpp"

namespace caffe {

template <typename Dtype>
class Net {
 public:
  inline void set_iter(int iter) { iter_ = iter; }
  int iter() { return iter_; }

 private:
  int iter_ = 0;
};

}  // namespace caffe
