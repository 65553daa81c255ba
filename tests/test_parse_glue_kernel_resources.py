"""Resource figures of k_parse_occ8 with the lean residual_coding glue (HIPDEC_PARSE_LEAN_GLUE), read from the code object in libheifhip.so (no GPU
needed): the shorter glue must not be paid for with more scratch, and the kernel stays on its occupancy step (64 VGPRs: 8 waves per SIMD; at most
5120 B of LDS: 32 one-wave workgroups per CU).  The kernel is looked up by its exact name: `k_parse_occ8` is also a prefix of k_parse_occ8_rf."""
import test_kernel_resources as R


def test_throughput_parser_budget_with_the_lean_glue():
    ks = R._kernels()
    hits = [v for k, v in ks.items() if "12k_parse_occ8E" in k]
    assert len(hits) == 1, sorted(ks)
    k = hits[0]
    # 188 B of scratch before the lean glue (profiles/parse_residual_glue.txt), 172 B with it
    assert k["vgpr"] <= 64 and k["lds"] <= 5120 and k["scratch"] <= 172, k
