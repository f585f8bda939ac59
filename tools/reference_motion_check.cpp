// Host sanitizer harness for reference-motion targets (mujocoposelearning_amd/csrc/hs_reward_prog.h): the
// validator with the two reference fields, the phase function and the host interpreter with a reference, the
// code a program that reads ref_qpos / ref_qvel passes through before it reaches the device.  Built with
// -fsanitize=address,undefined by `make -C mujocoposelearning_amd/csrc asan-reference-motion` and run by
// tests/test_reference_motion.py.
// For each file given: whitespace-separated tokens
//   nq nv nu nbody  n_instr n_consts n_params n_states  K key_dt flags fp32 seed
//   5 * n_instr code words, n_consts constants, n_params parameters,
//   n_states times ("nan" / "inf" / "-inf" allowed), n_states episode numbers,
//   K * nq qpos values, K * nv qvel values.
// The only state field such a program may read here is time.  Prints per file "OK <reward> ..." (one value per
// state, %.17g) or "ERR <message>".  Every state's phase is computed on its own as well and must give rows in
// [0, K - 1] and a weight in [0, 1): otherwise the line is "ERR phase ..." and the exit status is 1.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "hs_reward_prog.h"

int main(int argc, char** argv) {
  int status = 0;
  for (int a = 1; a < argc; a++) {
    std::ifstream in(argv[a]);
    hs::RpDims d{};
    long long n_instr = 0, n_consts = 0, n_params = 0, n_states = 0, K = 0, flags = 0, fp32 = 0;
    unsigned long long seed = 0;
    double key_dt = 0;
    if (!(in >> d.nq >> d.nv >> d.nu >> d.nbody >> n_instr >> n_consts >> n_params >> n_states >> K >> key_dt >> flags >>
          fp32 >> seed) ||
        d.nq < 1 || d.nv < 1 || d.nu < 0 || d.nbody < 0 || n_states < 0 || n_states > 100000 || K < 1 ||
        K > hs::RP_REF_MAX_ROWS) {
      std::printf("ERR cannot read the header of %s\n", argv[a]);
      continue;
    }
    auto count = [](long long n) { return (size_t)(n < 0 ? 0 : n > 1000000 ? 1000000 : n); };
    std::vector<int32_t> code(5 * count(n_instr));
    std::vector<double> consts(count(n_consts)), params(count(n_params));
    bool ok = true;
    for (auto& c : code) ok = ok && (in >> c);
    for (auto& c : consts) ok = ok && (in >> c);
    for (auto& c : params) ok = ok && (in >> c);
    auto number = [&](double& v) {
      std::string tok;   // "nan" / "inf" are not numbers to operator>>
      ok = ok && (in >> tok);
      if (ok) v = std::strtod(tok.c_str(), nullptr);
    };
    std::vector<double> time((size_t)n_states), q((size_t)K * d.nq), v((size_t)K * d.nv);
    std::vector<int32_t> episode((size_t)n_states);
    std::vector<uint64_t> seeds((size_t)n_states, (uint64_t)seed);
    for (auto& t : time) number(t);
    for (auto& e : episode) ok = ok && (in >> e);
    for (auto& x : q) number(x);
    for (auto& x : v) number(x);
    if (!ok) {
      std::printf("ERR %s is truncated\n", argv[a]);
      continue;
    }
    hs::RpInfo info;
    const std::string why =
        hs::rp_validate(d, code.data(), (int)n_instr, consts.data(), (int)n_consts, (int)n_params, &info);
    if (!why.empty()) {
      std::printf("ERR %s\n", why.c_str());
      continue;
    }
    if (info.fields & ~(hs::RP_REF_FIELDS | (1u << hs::RP_F_TIME))) {
      std::printf("ERR the harness supplies time and the reference only\n");
      continue;
    }
    if (K > 1 && !(key_dt > 0)) {
      std::printf("ERR key_dt must be > 0\n");
      continue;
    }
    bool phase_ok = true;
    for (long long s = 0; s < n_states && phase_ok; s++) {
      int i = -1, i1 = -1;
      const int j0 = hs::rp_ref_start((int)flags, (uint64_t)seed, (int)s, episode[(size_t)s], (int)K);
      const double w = hs::rp_ref_phase((int)K, (int)flags, j0, time[(size_t)s], key_dt, &i, &i1);
      if (j0 < 0 || j0 >= K || i < 0 || i >= K || i1 < 0 || i1 >= K || !(w >= 0.0 && w < 1.0)) {
        std::printf("ERR phase of state %lld: j0 %d i %d i1 %d w %.17g\n", s, j0, i, i1, w);
        phase_ok = false;
        status = 1;
      }
    }
    if (!phase_ok) continue;
    hs::RpRefHost ref;
    ref.K = (int)K;
    ref.qpos = q.data();
    ref.qvel = v.data();
    ref.key_dt = key_dt;
    ref.flags = (int)flags;
    ref.fp32 = fp32 != 0;
    ref.episode = episode.data();
    ref.seed = seeds.data();
    const double* fp[hs::RP_NFIELDS] = {};
    fp[hs::RP_F_TIME] = time.data();
    std::vector<double> out((size_t)n_states);
    hs::rp_eval_host(d, code.data(), (int)n_instr, consts.data(), params.data(), (int)n_states, fp, out.data(), nullptr,
                     &ref);
    std::printf("OK");
    for (double r : out) std::printf(" %.17g", r);
    std::printf("\n");
  }
  return status;
}
