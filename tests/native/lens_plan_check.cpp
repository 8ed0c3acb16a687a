// lens_plan_check.cpp — prints the batches job_plan.cpp plans for a lens render
// (rtnw::plan_lens, rtnw::lens_batch): `lens_plan_check NPIX SPP [KNOB]`, KNOB the text of
// RTNW_LENS_BATCH (absent: the default).  First line: the limit and the plan; then one line per
// batch: p0 np s0 ns.  Host arithmetic only; tests/test_lens_spec.py checks that every
// (pixel, sample) lands in exactly one batch.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "job_plan.h"

int rt_internal_fail(int code, const std::string &msg) {
    std::fprintf(stderr, "%s\n", msg.c_str());
    return code;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const uint64_t npix = std::strtoull(argv[1], nullptr, 10), spp = std::strtoull(argv[2], nullptr, 10);
    const uint64_t limit = rtnw::lens_batch_limit(argc > 3 ? argv[3] : nullptr);
    const rtnw::LensPlan pl = rtnw::plan_lens(npix, spp, limit);
    std::printf("%llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)limit, (unsigned long long)pl.pix_per,
                (unsigned long long)pl.smp_per, (unsigned long long)pl.nblocks, (unsigned long long)pl.nruns,
                (unsigned long long)pl.nbatches, (unsigned long long)pl.rays_per);
    for (uint64_t b = 0; b < pl.nbatches; b++) {
        const rtnw::LensBatch l = rtnw::lens_batch(pl, b, npix, spp);
        std::printf("%llu %llu %llu %llu\n", (unsigned long long)l.p0, (unsigned long long)l.np, (unsigned long long)l.s0,
                    (unsigned long long)l.ns);
    }
    return 0;
}
