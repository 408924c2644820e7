/* float64 sample loops of the Compressor and Limiter definitions (DESIGN.md "Dynamics FX"), compare / select form, on one host
 * core: the baseline profiles/r10_dynamics_fx.txt puts beside k_fx_dynamics.  gcc -O2 dynamics_fx_host.c -lm */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

static double cte(double ms, double fs) { return ms < 1e-3 ? 0.0 : exp(-2.0 * M_PI * 1000.0 / (ms * fs)); }

static void stage(const double *x, double *y, long n, double fs, double t_db, double ratio, double attack_ms, double release_ms) {
  const double T = pow(10.0, t_db / 20.0), slope = 1.0 / ratio - 1.0, cA = cte(attack_ms, fs), cR = cte(release_ms, fs);
  double e = 0.0;
  for (long t = 0; t < n; ++t) {
    const double a = fabs(x[t]);
    e = a + (a > e ? cA : cR) * (e - a);
    y[t] = (e < T ? 1.0 : pow(e / T, slope)) * x[t];
  }
}

static double now(void) {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

int main(void) {
  const double fs = 48000.0;
  const long lengths[3] = {192000, 480000, 2880000};
  for (int k = 0; k < 3; ++k) {
    const long n = lengths[k];
    float *x32 = malloc(n * sizeof(float)), *y32 = malloc(n * sizeof(float));
    double *x = malloc(n * sizeof(double)), *y1 = malloc(n * sizeof(double)), *y2 = malloc(n * sizeof(double));
    srand(1);
    for (long t = 0; t < n; ++t) x32[t] = (float)(rand() / (double)RAND_MAX - 0.5);
    double best_c = 1e9, best_l = 1e9, sink = 0.0;
    for (int rep = 0; rep < 5; ++rep) {
      double t0 = now();
      for (long t = 0; t < n; ++t) x[t] = x32[t];
      stage(x, y1, n, fs, -30.0, 4.0, 5.0, 120.0);
      for (long t = 0; t < n; ++t) y32[t] = (float)y1[t];
      double t1 = now();
      sink += y32[n / 2];
      best_c = t1 - t0 < best_c ? t1 - t0 : best_c;
      t0 = now();
      for (long t = 0; t < n; ++t) x[t] = x32[t];
      stage(x, y1, n, fs, -10.0, 4.0, 2.0, 200.0);
      stage(y1, y2, n, fs, -25.0, 1000.0, 0.0, 300.0);
      const double G = pow(10.0, 10.0 * 0.75 / 40.0) * pow(10.0, 25.0 / 20.0);
      for (long t = 0; t < n; ++t) y32[t] = (float)fmin(fmax(G * y2[t], -1.0), 1.0);
      t1 = now();
      sink += y32[n / 2];
      best_l = t1 - t0 < best_l ? t1 - t0 : best_l;
    }
    printf("host n=%ld: compressor %.2f ms, limiter %.2f ms (best of 5; checksum %g)\n", n, best_c * 1e3, best_l * 1e3, sink);
    free(x32); free(y32); free(x); free(y1); free(y2);
  }
  return 0;
}
