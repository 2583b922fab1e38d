// What tests/golden/make_rs_codes.py needs from libcorrect beyond its public functions: the order that
// correct_reed_solomon_decode's locator search left behind, which lives in the decoder's private struct (a word with zero syndromes
// returns before the search, so the recorder clears the order in front of every decode).  Built together with libcorrect's own
// reed-solomon sources into oracle/_ref/librs_ref.so (make -C oracle rs_ref); nothing of that library is kept here.
#include <correct/reed-solomon.h>

unsigned int rs_ref_locator_order(const correct_reed_solomon *rs) { return rs->error_locator.order; }
void rs_ref_clear_locator_order(correct_reed_solomon *rs) { rs->error_locator.order = 0; }
