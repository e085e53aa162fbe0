// The device self-tests: the library's hand-written device arithmetic on caller-supplied arguments (tests/test_gpu_device_math.py).
#include "ens.hpp"

extern "C" {

int rscm_gpu_selftest_normal(const uint64_t* k52, int64_t n, double* z)
{
    GUARD_BEGIN
    if (n < 0 || !k52 || !z) return fail(RSCM_ERR_INVALID, "bad arguments");
    if (n == 0) return RSCM_OK;
    rscm::DevBuf<double> buf;   // [n] integers, then [n] deviates
    HIPCHK(buf.alloc(2 * (size_t)n));
    double* d = buf.get();
    HIPCHK(hipMemcpy(d, k52, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIPCHK(rscm::launch_normal_selftest(reinterpret_cast<const uint64_t*>(d), n, d + n, nullptr));
    HIPCHK(hipMemcpy(z, d + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return RSCM_OK;
    GUARD_END
}

int rscm_gpu_selftest_math(int32_t op, int64_t n, const double* x, const double* y, double* out)
{
    GUARD_BEGIN
    const bool two = op == 3;   // pow_ratio reads y
    if (op < 0 || op >= rscm::kMathTestOps) return fail(RSCM_ERR_INVALID, "selftest_math: op %d is not in [0, %d)", op, rscm::kMathTestOps);
    if (n < 0 || !x || !out || (two && !y)) return fail(RSCM_ERR_INVALID, "bad arguments");
    if (n == 0) return RSCM_OK;
    rscm::DevBuf<double> buf;   // [n] x, [n] out, then [n] y for the two-argument op
    HIPCHK(buf.alloc((two ? 3 : 2) * (size_t)n));
    double* d = buf.get();
    HIPCHK(hipMemcpy(d, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    if (two) HIPCHK(hipMemcpy(d + 2 * n, y, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(rscm::launch_mathtest(op, d, two ? d + 2 * n : nullptr, d + n, n, nullptr));
    HIPCHK(hipMemcpy(out, d + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return RSCM_OK;
    GUARD_END
}

int rscm_gpu_selftest_div(int32_t device_id, int64_t n, const double* num, const double* den,
                          double* out_ref, double* out_fast, uint8_t* used_fast)
{
    GUARD_BEGIN
    if (n < 0 || !num || !den || !out_ref || !out_fast || !used_fast) return fail(RSCM_ERR_INVALID, "bad arguments");
    if (n == 0) return RSCM_OK;
    HIPCHK(hipSetDevice(device_id));
    rscm::DevBuf<double> buf;   // [n] num, den, out_ref, out_fast
    rscm::DevBuf<uint8_t> du;
    HIPCHK(buf.alloc(4 * (size_t)n));
    HIPCHK(du.alloc((size_t)n));
    double* d = buf.get();
    HIPCHK(hipMemcpy(d, num, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d + n, den, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(rscm::launch_divtest(d, d + n, d + 2 * n, d + 3 * n, du.get(), n, nullptr));
    HIPCHK(hipMemcpy(out_ref, d + 2 * n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_fast, d + 3 * n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(used_fast, du.get(), (size_t)n, hipMemcpyDeviceToHost));
    return RSCM_OK;
    GUARD_END
}

int rscm_gpu_selftest_pair_div(int32_t device_id, int64_t n, int32_t num_lo, const double* num, const double* den, double* out_ieee,
                               double* out_plain, double* out_verdict, int32_t* variant)
{
    GUARD_BEGIN
    if (n < 0 || !num || !den || !out_ieee || !out_plain || !out_verdict || !variant) return fail(RSCM_ERR_INVALID, "bad arguments");
    if (n == 0) return RSCM_OK;
    HIPCHK(hipSetDevice(device_id));
    rscm::DevBuf<double> buf;   // [n] num, den, ieee, plain, verdict
    rscm::DevBuf<int32_t> dv;
    HIPCHK(buf.alloc(5 * (size_t)n));
    HIPCHK(dv.alloc((size_t)n));
    double* d = buf.get();
    HIPCHK(hipMemcpy(d, num, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d + n, den, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(rscm::launch_pair_div_selftest(d, d + n, n, num_lo, d + 2 * n, d + 3 * n, d + 4 * n, dv.get(), nullptr));
    HIPCHK(hipMemcpy(out_ieee, d + 2 * n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_plain, d + 3 * n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_verdict, d + 4 * n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(variant, dv.get(), (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return RSCM_OK;
    GUARD_END
}

}  // extern "C"
