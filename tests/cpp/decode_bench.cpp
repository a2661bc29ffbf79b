// decode_bench -- wall time of CKKSEncoder::decode and Decryptor::decrypt through the SEAL surface.
//
//   decode_bench <label> [calls]
//
// At N = 2^16: decode at L = 1, 3, 17, 31 with full slots and at L = 17 with sparse_slots = 2^12,
// decrypt (size 2, followed by a stream synchronise) at L = 31.  Every shape runs 2 warm calls, then
// `calls` (default 7) timed ones; one raw line per call and one summary line (median, min, max) per
// shape, each starting with <label>, so two builds of the library can be alternated in one run and
// compared line by line.  Uses only the public SEAL API, so it builds against any revision.
// The max_err lines compare the decoded slots with the encoded values (for the sparse context
// against the input as given, which the sparse encoding does not reproduce slot for slot: there the
// figure only shows that two builds agree).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "seal/seal.h"

extern "C" int mhe_stream_sync(mhe_ctx *ctx, void *stream);

using namespace seal;

static double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

template <class F>
static void measure(const char *label, const std::string &shape, int calls, F &&f)
{
    for (int i = 0; i < 2; i++) f();
    std::vector<double> t;
    for (int i = 0; i < calls; i++)
    {
        const double t0 = now_ms();
        f();
        t.push_back(now_ms() - t0);
        std::printf("%s %s call=%d ms=%.4f\n", label, shape.c_str(), i, t.back());
    }
    std::sort(t.begin(), t.end());
    std::printf("%s %s median_ms=%.4f min_ms=%.4f max_ms=%.4f calls=%d\n", label, shape.c_str(), t[t.size() / 2],
                t.front(), t.back(), calls);
    std::fflush(stdout);
}

static void run_level(const char *label, int calls, int L, std::size_t sparse, bool with_decrypt)
{
    const std::size_t n = 65536;
    std::vector<int> bits{ 51 };
    for (int i = 1; i < L; i++) bits.push_back(46);
    bits.push_back(51); // special prime
    EncryptionParameters parms(scheme_type::ckks);
    parms.set_poly_modulus_degree(n);
    parms.set_coeff_modulus(CoeffModulus::Create(n, bits));
    if (sparse) parms.set_sparse_slots(sparse);
    SEALContext ctx(parms, true, sec_level_type::none);
    CKKSEncoder encoder(ctx);
    const std::size_t count = sparse ? sparse : n / 2;
    std::vector<double> v(count);
    for (std::size_t i = 0; i < count; i++) v[i] = std::sin(0.001 * (double)i);
    Plaintext pt;
    encoder.encode(v, 1099511627776.0, pt); // 2^40
    std::vector<std::complex<double>> out;
    const std::string shape = "decode N=65536 L=" + std::to_string(L) + " sparse=" + std::to_string(sparse);
    measure(label, shape, calls, [&] { encoder.decode(pt, out); });
    double err = 0;
    for (std::size_t i = 0; i < count; i++) err = std::max(err, std::abs(out[i] - v[i]));
    std::printf("%s %s max_err=%.3e\n", label, shape.c_str(), err);
    if (!with_decrypt) return;
    KeyGenerator keygen(ctx);
    Encryptor enc(ctx, keygen.secret_key());
    Decryptor dec(ctx, keygen.secret_key());
    Ciphertext ct;
    enc.encrypt_symmetric(pt, ct);
    Plaintext dp;
    measure(label, "decrypt N=65536 L=" + std::to_string(L) + " size=2", calls, [&] {
        dec.decrypt(ct, dp);
        mhe_stream_sync(ctx.engine(), ctx.stream());
    });
    encoder.decode(dp, out);
    err = 0;
    for (std::size_t i = 0; i < count; i++) err = std::max(err, std::abs(out[i] - v[i]));
    std::printf("%s decrypt N=65536 L=%d size=2 max_err=%.3e\n", label, L, err);
}

int main(int argc, char **argv)
{
    const char *label = argc > 1 ? argv[1] : "run";
    const int calls = argc > 2 ? std::max(5, std::atoi(argv[2])) : 7;
    for (int L : { 1, 3, 17, 31 }) run_level(label, calls, L, 0, L == 31);
    run_level(label, calls, 17, 4096, false);
    return 0;
}
