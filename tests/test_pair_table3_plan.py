"""Fold plan of the pair kernel with the three-core product tables (kernel_fiber_pair.hpp: PairMap<Model, K, true, true>,
Side::td() == 3; kernel_common.hpp: pair_tab3L_off / pair_tab3R_off).

A side of K with three cores or more takes its three outer cores from one table row per index triple instead of a two-core row and
a staged product.  Counted from PairMap::plan() for car7d, per tile:

    K                        0   1   2   3   4   5   6   sum
    staging rounds, now      4   3   2   2   2   3   4    20
    with three-core tables   3   2   1   0   1   2   3    12
    products, now           31  23  15  14  10  12  20   125
    with three-core tables  24  16   8   0   6   8  16    78

The two-core plan (PairMap<Model, K, true>, what every existing instantiation compiles) must not move, nor the slots, NV and the key
levels of the pre-pass.  The tables follow tabR in the arena, tab3L then tab3R, and are reserved only where a three-core
instantiation is registered and one table takes 16 MB at the most.

A syntax-only host pass over the headers; nothing is generated."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "c3sc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

TABLE3_PLAN_CHECKS = r"""
#include "launch_fpp.hpp"
#include "models.hpp"
using namespace c3sc;
typedef std::make_integer_sequence<int, 7> AllK;
// the two-core plan is what it was, and `true` keeps its meaning: PairMap<Model, K, true> is the two-core map
#define PLAN2(K, STAGED, PROD) \
    static_assert(PairMap<Car7D, K, true>::plan().staged == (STAGED) && PairMap<Car7D, K, true, false>::plan().staged == (STAGED), "car7d two-core staging rounds, K = " #K); \
    static_assert(PairMap<Car7D, K, true>::plan().products == (PROD) && PairMap<Car7D, K, true, false>::plan().products == (PROD), "car7d two-core products, K = " #K);
PLAN2(0, 4, 31)
PLAN2(1, 3, 23)
PLAN2(2, 2, 15)
PLAN2(3, 2, 14)
PLAN2(4, 2, 10)
PLAN2(5, 3, 12)
PLAN2(6, 4, 20)
// the three-core plan
#define PLAN3(K, STAGED, PROD) \
    static_assert(PairMap<Car7D, K, true, true>::plan().staged == (STAGED), "car7d three-core staging rounds, K = " #K); \
    static_assert(PairMap<Car7D, K, true, true>::plan().products == (PROD), "car7d three-core products, K = " #K);
PLAN3(0, 3, 24)
PLAN3(1, 2, 16)
PLAN3(2, 1, 8)
PLAN3(3, 0, 0)
PLAN3(4, 1, 6)
PLAN3(5, 2, 8)
PLAN3(6, 3, 16)
template <bool T3, int... Ks>
constexpr int products(std::integer_sequence<int, Ks...>) { return (PairMap<Car7D, Ks, true, T3>::plan().products + ...); }
template <bool T3, int... Ks>
constexpr int staged(std::integer_sequence<int, Ks...>) { return (PairMap<Car7D, Ks, true, T3>::plan().staged + ...); }
static_assert(products<false>(AllK{}) == 125 && products<true>(AllK{}) == 78, "car7d: products over a step");
static_assert(staged<false>(AllK{}) == 20 && staged<true>(AllK{}) == 12, "car7d: staging rounds over a step");
// without the edge tables the depth flag is inert
static_assert(PairMap<Car7D, 3, false, true>::plan().products == PairMap<Car7D, 3, false>::plan().products &&
              PairMap<Car7D, 3, false, true>::plan().staged == 6, "no edge tables: no three-core tables either");
// table depth per side: three where the side has three cores, two where it has two, none for a lone edge core
static_assert(PairMap<Car7D, 3, true, true>::SL::td() == 3 && PairMap<Car7D, 3, true, true>::SR::td() == 3, "K = 3: both sides");
static_assert(PairMap<Car7D, 2, true, true>::SL::td() == 2 && PairMap<Car7D, 2, true, true>::SR::td() == 3, "K = 2: two cores on the left");
static_assert(PairMap<Car7D, 1, true, true>::SL::td() == 0 && PairMap<Car7D, 0, true, true>::SL::td() == 0, "K = 0, 1: no table on the left");
static_assert(PairMap<Car7D, 3, true>::SL::td() == 2 && PairMap<Car7D, 3, false>::SL::td() == 0, "the two-core map and the map without tables");
// nothing of the node loop moves: NV, every item's slot, count and validity
template <int K>
constexpr bool same_slots()
{
    typedef PairMap<Car7D, K, true, true> P3;
    typedef PairMap<Car7D, K, true> P2;
    if (P3::nv() != P2::nv() || P3::SL::nv() != P2::SL::nv()) return false;
    for (int it = 0; it < P2::NIT; it++)
        if (P3::gslot(it) != P2::gslot(it) || P3::count(it) != P2::count(it) || P3::valid(it) != P2::valid(it)) return false;
    return true;
}
static_assert(same_slots<0>() && same_slots<1>() && same_slots<2>() && same_slots<3>() && same_slots<4>() && same_slots<5>() && same_slots<6>(),
              "car7d: nv() and gslot() with the three-core tables equal the two-core map's");
// the pre-pass keeps its key levels; a key level the tables absorb is no uniform round any more
static_assert(fpp_key_levels(7, 3, true).major == 2 && fpp_key_levels(7, 3, true).minor == 4 && fpp_key_levels(7, 0, true).major == 1 &&
              fpp_key_levels(7, 0, true).minor == 2, "car7d key levels");
static_assert(PairMap<Car7D, 3, true>::uniform_rounds() == 2 && PairMap<Car7D, 3, true, true>::uniform_rounds() == 0 &&
              PairMap<Car7D, 2, true, true>::uniform_rounds() == 1 && PairMap<Car7D, 0, true, true>::uniform_rounds() == 2, "uniform rounds left");
// a tile uniform in both keys stages level 3 only at K = 0 and K = 6, nothing at K = 1 .. 5
template <int K>
constexpr int rounds_left() { return PairMap<Car7D, K, true, true>::plan().staged - PairMap<Car7D, K, true, true>::uniform_rounds(); }
static_assert(rounds_left<0>() == 1 && rounds_left<6>() == 1 && rounds_left<1>() == 0 && rounds_left<2>() == 0 && rounds_left<3>() == 0 &&
              rounds_left<4>() == 0 && rounds_left<5>() == 0, "staging rounds of a tile uniform in both keys");
// registration and the opt-out list
static_assert(fpp_table3_registered(7, 10) && !fpp_table3_registered(7, 4) && !fpp_table3_registered(6, 10), "car7d at rank 10 only");
// arena layout: tabL, tabR, tab3L, tab3R in this order behind the last pair image, each on a 16-double boundary
constexpr bool layout(int n)
{
    KArgs A{};
    A.d = 7;
    long off = 1024;
    for (int m = 0; m < 7; m++) {
        A.ngrid[m] = n + m; // all different
        A.pair_img_off[m] = off;
        off += pair_img_doubles(n + m, (m == 0 || m == 6) ? 10 : 100);
    }
    const long tl = pair_tabL_off(A, 10), tr = pair_tabR_off(A, 10), t3l = pair_tab3L_off(A, 10), t3r = pair_tab3R_off(A, 10);
    return tl == off && tr == tl + pair_tab_doubles(n, n + 1, 10) && t3l == tr + pair_tab_doubles(n + 5, n + 6, 10) &&
           t3r == t3l + pair_tab3_doubles(n, n + 1, n + 2, 10) && tl % 16 == 0 && tr % 16 == 0 && t3l % 16 == 0 && t3r % 16 == 0 &&
           pair_tab3_doubles(n, n + 1, n + 2, 10) >= (long)n * (n + 1) * (n + 2) * 10;
}
static_assert(layout(5) && layout(41), "the table offsets in order inside the arena");
// the 16 MB rule
constexpr bool reserved(int n, int d = 7, int rp = 10)
{
    int ng[MAXD] = {};
    for (int m = 0; m < d; m++) ng[m] = n;
    return pair_tab3_reserved(d, ng, rp);
}
static_assert(reserved(41) && reserved(5) && !reserved(128), "reserved at N = 41 (5.5 MB a table), not at N = 128 (168 MB)");
static_assert(reserved(59) && !reserved(60), "59^3 rows of 80 bytes are 16.4e6 bytes, 60^3 are 17.3e6: the bound is 16 MiB");
static_assert(!reserved(41, 7, 4) && !reserved(41, 6, 8), "no three-core instantiation, no tables");
constexpr bool reserved_mixed()
{ // one table over the bound is enough to fall back to the two-core kernels
    int ng[MAXD] = {41, 41, 41, 41, 128, 128, 128};
    return pair_tab3_reserved(7, ng, 10);
}
static_assert(!reserved_mixed(), "the right table alone exceeds the bound");
int main() { return 0; }
"""


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_table3_plan_static_asserts(tmp_path):
    src = tmp_path / "table3_plan.hip"
    src.write_text(TABLE3_PLAN_CHECKS)
    r = subprocess.run([HIPCC, "-std=c++20", "--cuda-host-only", "-fsyntax-only", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
