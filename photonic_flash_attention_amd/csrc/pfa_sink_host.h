// pfa_sink_host.h -- what the entry-point files of the attention sinks share (pfa_decode_sink_capi.hip and the three
// pfa_prefill*_sink_capi.hip): the field rules of pfa_fa3_sinks and the place of "_sink" in a describe name.  Internal.
#pragma once
#include <stdio.h>
#include <string.h>

#include "pfa_host.h"

namespace pfa {

// include/pfa_hip.h, pfa_fa3_sinks, in the order the errors are reported; the caller has seen that the block is there (a NULL block is
// the sibling call).  pointers = false leaves out the two rules about `sinks` (a workspace query takes no pointers).
inline int check_sinks(const pfa_fa3_sinks* s, bool pointers = true) {
    if (s->size != sizeof(pfa_fa3_sinks)) return PFA_ERR_STRUCT_SIZE;
    if (s->flags != 0) return PFA_ERR_FLAGS;
    if (pointers) {
        if (!s->sinks) return PFA_ERR_NULL;
        if (!aligned4(s->sinks)) return PFA_ERR_ALIGN;
    }
    return PFA_OK;
}

// The sibling's describe name with "_sink" behind "_win" (or where that would stand): in front of "+combine", "_varlen", "_split{N}+merge"
// and "_paged", whichever comes first.  In place: buf holds the name on entry.
inline void name_sink(char* buf, size_t n) {
    if (!buf || !n) return;
    char name[128];
    snprintf(name, sizeof(name), "%s", buf);
    const char* at = name + strlen(name);
    for (const char* mark : {"+combine", "_varlen", "_split", "_paged"}) {
        const char* f = strstr(name, mark);
        if (f && f < at) at = f;
    }
    snprintf(buf, n, "%.*s_sink%s", (int)(at - name), name, at);
}

}  // namespace pfa
