// hipBLASLt entry points of lt_gemm.cpp that ops.cpp binds.  They take
// tensors, so they stay out of launchers.h, which the kernel files include.
#pragma once

#include <torch/extension.h>
#include <vector>

// x [N, D], w1 [F, D], b1 [F] bf16 -> gelu(x @ w1^T + b1) [N, F]
torch::Tensor lt_linear_gelu_bias(torch::Tensor x, torch::Tensor w1,
                                  torch::Tensor b1);
bool lt_probe_epilogue(long m, long n, long k, long epi);
// {algo_index, ms} pairs for the heuristic's top algos of a bf16 GEMM config
std::vector<double> lt_bench_algos(long m, long n, long k, bool ta, bool tb,
                                   long iters);
