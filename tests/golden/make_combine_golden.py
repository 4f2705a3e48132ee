"""Writes tests/golden/combine_ref_cases.npz: inputs and results of the reference's acceptance oracle for flash_attn_combine.

    python tests/golden/make_combine_golden.py /path/to/reference

The oracle is the function ``attention_combine_ref`` of the reference's hopper/test_flash_attn.py.  That module loads a GPU extension when imported, so the
function's definition is taken out of the PARSED source (ast) at generation time and compiled on its own; none of its text is stored here or in the fixture.
It runs on the CPU in fp32 on seeded inputs built the way the reference's test_flash_attn_combine builds them: out_partial as the first S of 2 S splits of
a transposed (.., H, L, D) tensor, lse_partial as the first H heads of a transposed (.., 2 H, L) tensor -- both non-contiguous -- and
lse_partial[S // 2:, :B // 3] = -inf, which for S = 1 leaves whole batch entries without a live split.

Per case `name`: name/out_partial (S, B, L, H, D) fp32, name/lse_partial (S, B, L, H) fp32, name/out (B, L, H, D) fp32, name/lse (B, L, H) fp32.
"""
import ast
import os
import sys

import numpy as np
import torch

# (S, L, D, H): every S, L and D of the list once at least, not the full product -- a case stays below 100 kB, so the large S meet the small L x D x H; B = 3
CASES = [(1, 113, 64, 1), (2, 113, 8, 2), (3, 113, 8, 1), (2, 3, 128, 4), (3, 1, 512, 2), (5, 3, 40, 2), (17, 3, 96, 1), (64, 1, 64, 1), (65, 3, 8, 2),
         (133, 1, 40, 1), (256, 1, 8, 2), (2, 3, 192, 2), (5, 3, 256, 1), (17, 1, 128, 2)]
B = 3


def reference_oracle(reference_root):
    path = os.path.join(reference_root, "hopper", "test_flash_attn.py")
    tree = ast.parse(open(path).read(), filename=path)
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "attention_combine_ref")
    ns = {"torch": torch}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return ns["attention_combine_ref"]


def main():
    ref = reference_oracle(sys.argv[1])
    arrays = {}
    for i, (S, L, D, H) in enumerate(CASES):
        torch.random.manual_seed(1 + i)
        out_partial = torch.randn(S * 2, B, H, L, D, dtype=torch.float32).transpose(2, 3)[:S]
        lse_partial = torch.randn(S, B, H * 2, L, dtype=torch.float32).transpose(-1, -2)[:, :, :, :H]
        lse_partial[S // 2:, :B // 3] = -float("inf")
        out, lse = ref(out_partial, lse_partial)
        name = f"s{S}_l{L}_d{D}_h{H}"
        arrays[f"{name}/out_partial"] = out_partial.contiguous().numpy()
        arrays[f"{name}/lse_partial"] = lse_partial.contiguous().numpy()
        arrays[f"{name}/out"] = out.contiguous().numpy()
        arrays[f"{name}/lse"] = lse.contiguous().numpy()
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "combine_ref_cases.npz")
    np.savez_compressed(dst, **arrays)
    print(dst, os.path.getsize(dst), "bytes,", len(CASES), "cases")


if __name__ == "__main__":
    main()
