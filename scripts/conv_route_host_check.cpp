// Walks the three family tables of csrc/conv_route.cpp on the host: every query and every dispatch / pack call, for every route value,
// both values of `transposed` and both batch-invariant modes, over a grid of descriptors (valid and invalid), with NULL blobs -- so every
// call ends at a check and nothing is launched.  Built with -fsanitize=address,undefined by scripts/conv_route_host_check.sh.
#include <cstdio>

#include "flownet2_hip.h"

int main() {
  const int channels[] = {0, 2, 3, 12, 24, 40, 64, 70, 128}, maps[][2] = {{5, 7}, {6, 8}, {17, 28}, {16, 24}, {65, 76}, {2, 3}};
  const int geoms[][3] = {{1, 1, 0}, {3, 1, 1}, {3, 2, 1}, {4, 2, 1}, {5, 2, 2}, {7, 2, 3}, {3, 0, 1}, {3, 1, -1}, {7, 2, 1}};
  long calls = 0, refused = 0;
  size_t sizes = 0;
  for (int inv = 0; inv < 2; ++inv) {
    fn2_set_batch_invariant(inv);
    for (int N : {1, 8})
      for (int Cin : channels)
        for (int Cout : channels)
          for (const auto& m : maps)
            for (const auto& g : geoms) {
              const fn2_conv_desc d = {N, Cin, m[0], m[1], Cout, g[0], g[1], g[2]};
              for (int f = 0; f < 8; ++f) sizes += fn2_conv_route(&d, f) + fn2_deconv_route(&d, f);
              for (int a = 0; a <= 0x100; a += 0x100)
                for (int base = 0; base < 7; ++base) {
                  const int r = base | a;
                  sizes += fn2_conv_packed_weight_floats(&d, r) + fn2_conv_workspace_bytes(&d, r) + fn2_deconv_packed_weight_floats(&d, r) +
                           fn2_deconv_workspace_bytes(&d, r);
                  refused += fn2_conv_forward(&d, r, nullptr, Cin, 0, nullptr, nullptr, nullptr, Cout, 0, 1, 0.1f, nullptr, 0, nullptr) != FN2_OK;
                  refused += fn2_deconv_forward(&d, r, nullptr, Cin, 0, nullptr, nullptr, nullptr, Cout, 0, 0, 0.1f, nullptr, 0, nullptr) != FN2_OK;
                  refused += fn2_conv_pack_weights(&d, r, nullptr, nullptr, nullptr) != FN2_OK;
                  refused += fn2_deconv_pack_weights(&d, r, nullptr, nullptr, nullptr) != FN2_OK;
                  for (int tr = 0; tr < 2; ++tr) {
                    const int Cp = fn2_conv_backward_data_computed_channels(&d, tr, r);
                    sizes += fn2_conv_backward_data_packed_weight_floats(&d, tr, r) + fn2_conv_backward_data_pack_workspace_bytes(&d, tr, r) +
                             fn2_conv_backward_data_workspace_bytes(&d, tr, r) + fn2_conv_backward_data_workspace_bytes_with_room(&d, tr, r, Cin) +
                             fn2_conv_backward_data_workspace_bytes_with_room(&d, tr, r, Cp) + fn2_conv_backward_data_masked_supported(&d, tr, r) +
                             fn2_conv_backward_weights_workspace_bytes_arith(&d, tr, r);
                    refused += fn2_conv_backward_data_pack_weights(&d, tr, r, nullptr, nullptr, nullptr, 0, nullptr) != FN2_OK;
                    refused += fn2_conv_backward_data(&d, tr, r, nullptr, Cout, 0, nullptr, nullptr, Cin, 0, Cin, nullptr, 0, nullptr) != FN2_OK;
                    refused += fn2_conv_backward_data_masked(&d, tr, r, nullptr, Cout, 0, nullptr, nullptr, Cin, 0, nullptr, Cin, 0, 0.1f, nullptr) != FN2_OK;
                    refused += fn2_conv_backward_weights_arith_run(&d, tr, r, nullptr, Cin, 0, nullptr, Cout, 0, nullptr, 0, nullptr, 0, nullptr) != FN2_OK;
                    calls += 4;
                  }
                  calls += 4;
                }
              for (int tr = 0; tr < 2; ++tr) {
                sizes += fn2_conv_backward_data_route(&d, tr) + fn2_conv_backward_data_route_flags(&d, tr, 2) + fn2_conv_backward_weights_supported(&d, tr) +
                         fn2_conv_backward_weights_workspace_bytes(&d, tr) + fn2_conv_backward_weights_bias_fused(&d, tr) + fn2_conv_backward_weights_arith(&d, tr, 2);
                refused += fn2_conv_backward_weights(&d, tr, nullptr, Cin, 0, nullptr, Cout, 0, nullptr, 0, nullptr, 0, nullptr) != FN2_OK;
                refused += fn2_conv_backward_weights_bias(&d, tr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr) != FN2_OK;
                calls += 2;
              }
            }
  }
  fn2_set_batch_invariant(0);
  std::printf("conv_route host check: %ld dispatch and pack calls on NULL blobs, %ld refused, size checksum %zu\n", calls, refused, sizes);
  return calls == refused ? 0 : 1;      // every one of them must have been refused on the host
}
