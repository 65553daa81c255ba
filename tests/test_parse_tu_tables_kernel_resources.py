"""Resource figures of k_parse_occ8 with the TU tables (HIPDEC_PARSE_TU_TABLES), read from the code object in libheifhip.so (no GPU needed): the
tables take LDS - 5120 B are four 1280-byte granules, 32 one-wave workgroups still fit a CU -, and must not be paid for with registers (64 VGPRs:
8 waves per SIMD) or with more scratch than the kernel had without them (148 B).  The kernel is looked up by its exact name."""
import test_kernel_resources as R


def test_throughput_parser_budget_with_the_tu_tables():
    ks = R._kernels()
    hits = [v for k, v in ks.items() if "12k_parse_occ8E" in k]
    assert len(hits) == 1, sorted(ks)
    k = hits[0]
    assert k["vgpr"] <= 64 and k["scratch"] <= 148 and k["lds"] <= 5120, k
