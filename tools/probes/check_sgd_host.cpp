// Host-only walk through check_sgd and make_sgd_args of csrc/train_rules.h: every refusal torch.optim.SGD makes and one acceptance.  It
// launches nothing and links against no GPU runtime; build it as plain C++ with the sanitizers on and run it:
//   clang++ -x c++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I$ROCM_PATH/include -fsanitize=address,undefined -fno-sanitize-recover=all \
//           tools/probes/check_sgd_host.cpp -o check_sgd_host.bin && ./check_sgd_host.bin
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../clip_calibration_amd/csrc/train_rules.h"

static char g_error[256];
void clipmi::set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
}

static int failures = 0;
static void expect(const char* what, float momentum, float dampening, float weight_decay, int nesterov, int code, const char* word) {
  g_error[0] = 0;
  const int rc = clipmi::check_sgd("probe", momentum, dampening, weight_decay, nesterov);
  const bool ok = rc == code && (code == CLIPMI_OK ? g_error[0] == 0 : strncmp(g_error, "probe: ", 7) == 0 && strstr(g_error, word) != nullptr);
  printf("%-34s rc=%d %s%s\n", what, rc, ok ? "ok" : "FAILED: ", ok ? "" : g_error);
  failures += !ok;
}

int main() {
  const float inf = INFINITY, nan = NAN;
  expect("momentum < 0", -0.1f, 0.f, 0.f, 0, CLIPMI_ERR_ARG, "momentum");
  expect("momentum = 1", 1.f, 0.f, 0.f, 0, CLIPMI_ERR_ARG, "momentum");
  expect("momentum NaN", nan, 0.f, 0.f, 0, CLIPMI_ERR_ARG, "momentum");
  expect("dampening < 0", 0.9f, -0.1f, 0.f, 0, CLIPMI_ERR_ARG, "dampening");
  expect("dampening = 1", 0.9f, 1.f, 0.f, 0, CLIPMI_ERR_ARG, "dampening");
  expect("dampening NaN", 0.9f, nan, 0.f, 0, CLIPMI_ERR_ARG, "dampening");
  expect("weight decay < 0", 0.9f, 0.f, -1e-4f, 0, CLIPMI_ERR_ARG, "weight_decay");
  expect("weight decay infinite", 0.9f, 0.f, inf, 0, CLIPMI_ERR_ARG, "weight_decay");
  expect("weight decay NaN", 0.9f, 0.f, nan, 0, CLIPMI_ERR_ARG, "weight_decay");
  expect("nesterov without a momentum", 0.f, 0.f, 0.f, 1, CLIPMI_ERR_ARG, "nesterov");
  expect("nesterov with dampening", 0.9f, 0.1f, 0.f, 1, CLIPMI_ERR_ARG, "nesterov");
  expect("plain SGD", 0.f, 0.f, 0.f, 0, CLIPMI_OK, "");
  expect("momentum, dampening, weight decay", 0.9f, 0.1f, 5e-4f, 0, CLIPMI_OK, "");
  expect("nesterov", 0.9f, 0.f, 5e-4f, 1, CLIPMI_OK, "");
  const clipmi::SgdArgs a = clipmi::make_sgd_args(0.9f, 0.1f, 5e-4f, 7, 3);
  const bool ok = a.momentum == 0.9f && a.one_minus_dampening == (float)(1.0 - (double)0.1f) && a.weight_decay == 5e-4f && a.nesterov == 1 && a.first_step == 1;
  printf("%-34s %s\n", "make_sgd_args", ok ? "ok" : "FAILED");
  failures += !ok;
  return failures ? 1 : 0;
}
