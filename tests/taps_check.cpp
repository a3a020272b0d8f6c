// Host check of sdr-j-fm_amd/csrc/fmx_taps.h (run by tests/test_taps_cpu.py): one query per line on stdin, one JSON object per query on stdout.  The program
// keeps ONE RecordTap and ONE SlotTap; the queries are their functions, in the order the host files call them.
//   r_init channels | r_start channels | r_user c on | r_switches          -> the tap's state
//   r_begin c pos                                                          -> {"job": 0 | 1} and the state
//   r_produced c n | r_on_from c pos   (what a stage stores behind its *_produce; stage_rds_meter stores rdsm::piece's on_from too)
//   r_take c ring capacity | r_read c ring capacity (take, then commit)    -> {"from": f, "count": n, "next": x, "want": ring_take's} and the state
//   s_init units | s_start units ring | s_user u value | s_switches | s_grow (cap = slots + slots_needed, then assign_slots) | s_restart
//   s_begin u pos | s_restart_unit u | s_tag u item | s_live v | s_commit u next     -> the tap's state (s_begin: with "job")
//   s_needed                                                               -> {"needed": n}
//   s_pending u capacity                                                   -> {"items": [...]}
//   s_run u capacity                                                       -> {"from": f, "count": n}
#include "../sdr-j-fm_amd/csrc/fmx_taps.h"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
using namespace fmx;

template <class V> static void list(const char *name, const V &v, const char *end = ", ") {
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); i++) printf("%s%lld", i ? ", " : "", (long long)v[i]);
    printf("]%s", end);
}
static void state(const RecordTap &t) {
    list("user", t.user); list("call", t.call); list("on_from", t.on_from); list("produced", t.produced); list("cursor", t.cursor);
    printf("\"alloc\": %d}\n", t.alloc ? 1 : 0);
}
static void state(const SlotTap &t) {
    list("user", t.user); list("call", t.call); list("slot", t.slot); list("on_from", t.on_from); list("cursor", t.cursor); list("tags", t.tags);
    printf("\"ring\": %d, \"slots\": %d, \"cap\": %d, \"live\": %d}\n", t.ring, t.slots, t.cap, t.live ? 1 : 0);
}

int main() {
    RecordTap R;
    SlotTap S;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string q;
        long long a = 0, b = 0, c = 0;
        in >> q >> a >> b >> c;
        printf("{");
        if (q == "r_init") { R.init((size_t)a); state(R); }
        else if (q == "r_start") { R.start((size_t)a); state(R); }
        else if (q == "r_user") { R.user[(size_t)a] = b != 0; state(R); }
        else if (q == "r_switches") { R.take_switches(); state(R); }
        else if (q == "r_begin") { printf("\"job\": %d, ", R.begin((size_t)a, b) ? 1 : 0); state(R); }
        else if (q == "r_produced") { R.produced[(size_t)a] = b; state(R); }
        else if (q == "r_on_from") { R.on_from[(size_t)a] = b; state(R); }
        else if (q == "r_take" || q == "r_read") {
            const RingTake want = ring_take(R.produced[(size_t)a], R.cursor[(size_t)a], b, c), t = R.take((size_t)a, b, c);
            if (q == "r_read") R.commit((size_t)a, t);
            printf("\"from\": %lld, \"count\": %lld, \"next\": %lld, \"want\": [%lld, %lld, %lld], ", (long long)t.from, (long long)t.count, (long long)t.next(),
                   (long long)want.from, (long long)want.count, (long long)want.next());
            state(R);
        }
        else if (q == "s_init") { S = SlotTap(); S.init((size_t)a); state(S); }
        else if (q == "s_start") { S.start((size_t)a, (int32_t)b); state(S); }
        else if (q == "s_user") { S.user[(size_t)a] = (int32_t)b; state(S); }
        else if (q == "s_switches") { S.take_switches(); state(S); }
        else if (q == "s_grow") { S.cap = S.slots + S.slots_needed(); S.assign_slots(); state(S); }
        else if (q == "s_restart") { S.restart(); state(S); }
        else if (q == "s_begin") { printf("\"job\": %d, ", S.begin((size_t)a, b) ? 1 : 0); state(S); }
        else if (q == "s_restart_unit") { S.restart_unit((size_t)a); state(S); }
        else if (q == "s_tag") { S.tag((size_t)a, b, b % S.ring); state(S); }
        else if (q == "s_live") { S.live = a != 0; state(S); }
        else if (q == "s_commit") { S.commit((size_t)a, b); state(S); }
        else if (q == "s_needed") printf("\"needed\": %d}\n", S.slots_needed());
        else if (q == "s_pending") { std::vector<int64_t> v; S.pending((size_t)a, b, v); list("items", v, "}\n"); }
        else if (q == "s_run") { const SlotRun r = S.run((size_t)a, b); printf("\"from\": %lld, \"count\": %d}\n", (long long)r.from, r.count); }
        else printf("\"error\": \"unknown query\"}\n");
    }
    return 0;
}
