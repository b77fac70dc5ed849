"""The case table of the fusion net's forward plan: the smallest shapes at which each decision of the plan flips, and the launch
sequence of each - RECORDED from ojf_net_profile of the commit before the plan existed (tools/net_sha.py on an MI355X, every row
in both arithmetics; the switch row in a child process), never from ojf_net_plan.  Shared by tests/test_net_plan_host.py
(ojf_net_plan against this table, no GPU) and tests/test_net_gpu.py (ojf_net_profile against ojf_net_plan).
Keys: version, use_semantics, n_points, growth (as the C ABI counts it: growth_factor - 1), h, w, arithmetic."""
CHAIN, PAIR = ['dense_chain_kernel'], ['dense_pair_kernel']
CONV16, GROUPED, CONV32 = ['conv_f16x3_kernel'], ['conv_f16x3_kernel (grouped)'], ['conv_mfma_kernel']
COLSUM, GAVE, ENTRY, PYRAMID = ['colsum_kernel'], ['gave_bias_kernel'], ['entry1x1_kernel'], ['pool_pyramid_kernel']
TAIL, TAIL_ENTRY = ['vortex_tail_kernel'], ['vortex_tail_kernel (+ next entry GEMM)']
TAIL_HALF, TAIL_HEAD = ['vortex_tail_kernel (+ half of the next entry GEMM)'], ['vortex_tail_kernel (+ prediction head)']

# What the rows reach:
#   9 points, growth 5 (the reference), v3: 24x32 the default chain flow; 45x77 w % 8 != 0 -> pair kernels and plain planes; 5x7 a
#   frame smaller than a tile; with semantics two heads, half-entry tails, colsum3, Q0; v2 without / with semantics: chain_kind 19 / 20
#   5/4, 3/3, 7/5 (and 5/3, 3/2, 7/4: the topologies of test_fusion_net_other_topologies, whose `growth` is growth_factor) at 40x56:
#   the general flow, unfused tail, layer-by-layer head; 5/4 at 160x208: npix >= 32768 -> branch 0 on the side stream
#   8/6 at 40x56: 140 input channels -> 16-tile stand-alone entry1x1_kernel, fused tail carrying the next entry GEMM, no chain-form head
PLANS = {
    (3, 0, 9, 5, 24, 32, 'f16x3'): CHAIN + ENTRY + PYRAMID + GROUPED * 2 + TAIL_ENTRY + PYRAMID + GROUPED * 2 + TAIL_HEAD,
    (3, 0, 9, 5, 24, 32, 'f32'): CONV32 * 10 + ENTRY + PYRAMID + CONV32 * 2 + TAIL_ENTRY + PYRAMID + CONV32 * 2 + TAIL_HEAD,
    (3, 0, 9, 5, 45, 77, 'f16x3'): PAIR * 5 + ENTRY + PYRAMID + GROUPED * 2 + TAIL_ENTRY + PYRAMID + GROUPED * 2 + TAIL_HEAD,
    (3, 0, 9, 5, 45, 77, 'f32'): CONV32 * 10 + ENTRY + PYRAMID + CONV32 * 2 + TAIL_ENTRY + PYRAMID + CONV32 * 2 + TAIL_HEAD,
    (3, 0, 9, 5, 5, 7, 'f16x3'): PAIR * 5 + ENTRY + PYRAMID + GROUPED * 2 + TAIL_ENTRY + PYRAMID + GROUPED * 2 + TAIL_HEAD,
    (3, 0, 9, 5, 5, 7, 'f32'): CONV32 * 10 + ENTRY + PYRAMID + CONV32 * 2 + TAIL_ENTRY + PYRAMID + CONV32 * 2 + TAIL_HEAD,
    (3, 1, 9, 5, 24, 32, 'f16x3'): CHAIN + ENTRY + PYRAMID + GROUPED * 2 + TAIL_HALF + CHAIN + ENTRY + PYRAMID + GROUPED * 2 + TAIL_HALF + PYRAMID + GROUPED * 2 + TAIL_HEAD,
    (3, 1, 9, 5, 24, 32, 'f32'): CONV32 * 10 + ENTRY + PYRAMID + CONV32 * 2 + TAIL_HALF + CONV32 * 10 + ENTRY + PYRAMID + CONV32 * 2 + TAIL_HALF + PYRAMID + CONV32 * 2 + TAIL_HEAD,
    (3, 1, 9, 5, 45, 77, 'f16x3'): PAIR * 5 + ENTRY + PYRAMID + GROUPED * 2 + TAIL_HALF + PAIR * 5 + ENTRY + PYRAMID + GROUPED * 2 + TAIL_HALF + PYRAMID + GROUPED * 2 + TAIL_HEAD,
    (3, 1, 9, 5, 45, 77, 'f32'): CONV32 * 10 + ENTRY + PYRAMID + CONV32 * 2 + TAIL_HALF + CONV32 * 10 + ENTRY + PYRAMID + CONV32 * 2 + TAIL_HALF + PYRAMID + CONV32 * 2 + TAIL_HEAD,
    (2, 0, 9, 5, 24, 32, 'f16x3'): CHAIN + ENTRY + PYRAMID + GROUPED * 2 + TAIL_ENTRY + PYRAMID + GROUPED * 2 + TAIL_HEAD,
    (2, 0, 9, 5, 24, 32, 'f32'): CONV32 * 10 + ENTRY + PYRAMID + CONV32 * 2 + TAIL_ENTRY + PYRAMID + CONV32 * 2 + TAIL_HEAD,
    (2, 1, 9, 5, 24, 32, 'f16x3'): CHAIN + ENTRY + PYRAMID + GROUPED * 2 + TAIL_ENTRY + PYRAMID + GROUPED * 2 + TAIL_HEAD,
    (2, 1, 9, 5, 24, 32, 'f32'): CONV32 * 10 + ENTRY + PYRAMID + CONV32 * 2 + TAIL_ENTRY + PYRAMID + CONV32 * 2 + TAIL_HEAD,
    (3, 0, 5, 4, 40, 56, 'f16x3'): PAIR * 4 + COLSUM + GAVE + CONV16 + PYRAMID + GROUPED * 2 + CONV16 * 5 + COLSUM + GAVE + CONV16 + PYRAMID + GROUPED * 2 + CONV16 * 14,
    (3, 0, 5, 4, 40, 56, 'f32'): CONV32 * 8 + COLSUM + GAVE + CONV32 + PYRAMID + CONV32 * 7 + COLSUM + GAVE + CONV32 + PYRAMID + CONV32 * 16,
    (3, 1, 3, 3, 40, 56, 'f16x3'): PAIR * 3 + COLSUM + GAVE + CONV16 + PYRAMID + GROUPED * 2 + CONV16 * 5 + PAIR * 3 + COLSUM + GAVE + CONV16 + PYRAMID + GROUPED * 2 + CONV16 * 5 + COLSUM + GAVE + CONV16 + PYRAMID + GROUPED * 2 + CONV16 * 12,
    (3, 1, 3, 3, 40, 56, 'f32'): CONV32 * 6 + COLSUM + GAVE + CONV32 + PYRAMID + CONV32 * 13 + COLSUM + GAVE + CONV32 + PYRAMID + CONV32 * 7 + COLSUM + GAVE + CONV32 + PYRAMID + CONV32 * 14,
    (2, 1, 7, 5, 40, 56, 'f16x3'): PAIR * 5 + COLSUM + GAVE + CONV16 + PYRAMID + GROUPED * 2 + CONV16 * 5 + COLSUM + GAVE + CONV16 + PYRAMID + GROUPED * 2 + CONV16 * 16,
    (2, 1, 7, 5, 40, 56, 'f32'): CONV32 * 10 + COLSUM + GAVE + CONV32 + PYRAMID + CONV32 * 7 + COLSUM + GAVE + CONV32 + PYRAMID + CONV32 * 18,
    (3, 0, 5, 3, 40, 56, 'f16x3'): PAIR * 3 + COLSUM + GAVE + CONV16 + PYRAMID + GROUPED * 2 + CONV16 * 5 + COLSUM + GAVE + CONV16 + PYRAMID + GROUPED * 2 + CONV16 * 12,
    (3, 0, 5, 3, 40, 56, 'f32'): CONV32 * 6 + COLSUM + GAVE + CONV32 + PYRAMID + CONV32 * 7 + COLSUM + GAVE + CONV32 + PYRAMID + CONV32 * 14,
    (3, 1, 3, 2, 40, 56, 'f16x3'): PAIR * 2 + COLSUM + GAVE + CONV16 + PYRAMID + GROUPED * 2 + CONV16 * 5 + PAIR * 2 + COLSUM + GAVE + CONV16 + PYRAMID + GROUPED * 2 + CONV16 * 5 + COLSUM + GAVE + CONV16 + PYRAMID + GROUPED * 2 + CONV16 * 10,
    (3, 1, 3, 2, 40, 56, 'f32'): CONV32 * 4 + COLSUM + GAVE + CONV32 + PYRAMID + CONV32 * 11 + COLSUM + GAVE + CONV32 + PYRAMID + CONV32 * 7 + COLSUM + GAVE + CONV32 + PYRAMID + CONV32 * 12,
    (2, 1, 7, 4, 40, 56, 'f16x3'): PAIR * 4 + COLSUM + GAVE + CONV16 + PYRAMID + GROUPED * 2 + CONV16 * 5 + COLSUM + GAVE + CONV16 + PYRAMID + GROUPED * 2 + CONV16 * 14,
    (2, 1, 7, 4, 40, 56, 'f32'): CONV32 * 8 + COLSUM + GAVE + CONV32 + PYRAMID + CONV32 * 7 + COLSUM + GAVE + CONV32 + PYRAMID + CONV32 * 16,
    (3, 0, 5, 4, 160, 208, 'f16x3'): PAIR * 4 + COLSUM + GAVE + CONV16 + PYRAMID + CONV16 * 2 + GROUPED * 2 + CONV16 * 5 + COLSUM + GAVE + CONV16 + PYRAMID + CONV16 * 2 + GROUPED * 2 + CONV16 * 14,
    (3, 0, 5, 4, 160, 208, 'f32'): CONV32 * 8 + COLSUM + GAVE + CONV32 + PYRAMID + CONV32 * 9 + COLSUM + GAVE + CONV32 + PYRAMID + CONV32 * 18,
    (3, 0, 8, 6, 40, 56, 'f16x3'): CHAIN + ENTRY + PYRAMID + GROUPED * 2 + TAIL_ENTRY + PYRAMID + GROUPED * 2 + TAIL + CONV16 * 13,
    (3, 0, 8, 6, 40, 56, 'f32'): CONV32 * 12 + ENTRY + PYRAMID + CONV32 * 2 + TAIL_ENTRY + PYRAMID + CONV32 * 2 + TAIL + CONV32 * 13,
}

# (3, 0, 9, 5, 24, 32, 'f16x3') under the test-only switch (read once per process)
SWITCH_PLANS = {
    'OJF_NO_DENSE_CHAIN': PAIR * 5 + ENTRY + PYRAMID + GROUPED * 2 + TAIL_ENTRY + PYRAMID + GROUPED * 2 + TAIL_HEAD,
}
