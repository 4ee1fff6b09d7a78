"""The shape grid of wide handles (crux_mlp_create_wide: a dimension above 1024), shared by tests/test_wide_reference.py (CPU) and tests/test_gpu_wide.py.

Each member reaches a place where the dense engine could break past 1024:
  1025-17 i  B 5     K = 1025 is no multiple of 4 or 16 (the dword operand path), one layer, one column tile
  1040-1030-3 B 33   both dimensions past 1024; dW of layer 0 has 65 x 65 = 4225 tiles, past launch_gemm's 4096-tile split-K limit
  2048-256-6 B 32/1  the head of examples/rl/atari.jl (wide as K of the forward and as M of the input gradient), at its batch and at one column
  3136-512-6 B 16    the head of the 84 x 84 DQN trunk; dW of layer 0 has 32 x 196 = 6272 tiles
  4096-16-2 t B 17   the cap, as K
  8-2048-4   B 33    wide as M of the forward and as K of the second layer and of the input gradient
  1024-1025-2 t B 15 just past the limit, as M (odd) and as K
"""
RELU2, TANH2 = ["relu", "identity"], ["tanh", "identity"]

WIDE_CASES = [([1025, 17], ["identity"], 5), ([1040, 1030, 3], RELU2, 33), ([2048, 256, 6], RELU2, 32), ([2048, 256, 6], RELU2, 1), ([3136, 512, 6], RELU2, 16),
              ([4096, 16, 2], TANH2, 17), ([8, 2048, 4], RELU2, 33), ([1024, 1025, 2], TANH2, 15)]
