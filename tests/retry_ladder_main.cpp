// Stand-alone driver of the retry ladder (csrc/rips_retry.h) for tests/test_retry_ladder.py: host
// C++ only.  First line: the error-flag values.  Then, for every line of ten integers on stdin
//     errs par_code force_global scale force_big no_par no_cap big par_strict reduce_wave
// one line "what force_global scale force_big no_par no_cap" (what: done, fail or retry; the
// attempt is the next one after retry, else the current one).
#include <cstdio>

#include "rips_retry.h"

int main() {
    using namespace tda;
    printf("%d %d %d %d %d %d %d %d %d %d %d\n", ERR_RESID_CAP, ERR_PAIR_CAP, ERR_WORK_CAP, ERR_VPOOL_CAP, ERR_OUT_CAP, ERR_LDS_SPILL,
           ERR_STEP_LIMIT, ERR_PAR, ERR_PAR2, ERR_CAP_MISS, kMaxParScale);
    int errs, fg, scale, fb, no_par, no_cap, big, strict, wave;
    unsigned code;
    while (scanf("%d %u %d %d %d %d %d %d %d %d", &errs, &code, &fg, &scale, &fb, &no_par, &no_cap, &big, &strict, &wave) == 10) {
        Attempt at;
        at.force_global = fg != 0;
        at.scale = scale;
        at.force_big = fb != 0;
        at.no_par = no_par;
        at.no_cap = no_cap != 0;
        const RetryStep st = next_attempt(errs, code, at, big != 0, strict != 0, wave != 0);
        static const char* names[] = {"done", "fail", "retry"};
        printf("%s %d %d %d %d %d\n", names[st.what], (int)st.next.force_global, st.next.scale, (int)st.next.force_big, st.next.no_par,
               (int)st.next.no_cap);
    }
    return 0;
}
