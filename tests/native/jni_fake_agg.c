/*
 * readGrouped of the JNI shim (jni/sgx_jni.c) with a reducing aggregation, on a host without a
 * JVM or a GPU (tests/test_jni_shim_agg.py): the fake JNIEnv of jni_fake_env.c, and a recording
 * stand-in for the two engine calls readGrouped makes.  The shim library defines them itself,
 * so its forwards bind here (linked -Bsymbolic) instead of to libsgx.so.
 */
#include "jni_fake_env.c"

#include <sgx.h>

static int64_t g_seen[8]; /* agg, keys NULL, group_starts NULL, values NULL, cap_groups, cap_values, start, end */

int sgx_read_grouped(sgx_engine *e, int32_t shuffle_id, const int64_t *map_ids, int64_t nmaps, int32_t start_partition,
                     int32_t end_partition, int32_t agg, int64_t *keys, int64_t *group_starts, int64_t *values,
                     int64_t cap_groups, int64_t cap_values, int32_t mem_kind, int64_t *out_groups,
                     int64_t *out_values) {
    (void)e;
    (void)shuffle_id;
    (void)map_ids;
    (void)mem_kind;
    const int64_t seen[8] = {agg, !keys, !group_starts, !values, cap_groups, cap_values, start_partition, end_partition};
    memcpy(g_seen, seen, sizeof seen);
    /* two groups per map id; a reducing aggregation has one value per group */
    *out_groups = 2 * nmaps;
    *out_values = agg == SGX_AGG_GROUP ? 5 * nmaps : 2 * nmaps;
    if (!keys && cap_groups == 0 && cap_values == 0) return SGX_OK; /* size query */
    if (*out_groups > cap_groups || *out_values > cap_values) return SGX_ERR_INVALID;
    for (int64_t g = 0; g < *out_groups; ++g) {
        keys[g] = 100 + g;
        if (group_starts) group_starts[g] = g; /* NULL for a caller that passes no starts buffer */
    }
    for (int64_t v = 0; v < *out_values; ++v) values[v] = -7 - v;
    return SGX_OK;
}

int sgx_last_read_records(sgx_engine *e, int64_t *out_records) {
    (void)e;
    *out_records = 42;
    return SGX_OK;
}

jlongArray Java_org_apache_spark_shuffle_ucx_gpu_SgxNative_readGrouped(JNIEnv *, jclass, jlong, jint, jlongArray, jint,
                                                                      jint, jint, jobject, jobject, jobject);

/* readGrouped over `nmaps` maps and partitions [1, 3); a NULL array = Java null for that buffer.
 * out3 = {groups, values, records}; seen8 = what the engine was called with.  -1 for Java null. */
int fake_read_grouped(int agg, int nmaps, int64_t *keys, int64_t keys_bytes, int64_t *starts, int64_t starts_bytes,
                      int64_t *values, int64_t values_bytes, int64_t *out3, int64_t *seen8) {
    obj k = {K_DIRECT, 0, keys, keys_bytes}, s = {K_DIRECT, 0, starts, starts_bytes},
        v = {K_DIRECT, 0, values, values_bytes};
    obj *m = new_obj(K_LONGS, nmaps, 8);
    memset(g_seen, 0xFF, sizeof g_seen);
    obj *r = (obj *)Java_org_apache_spark_shuffle_ucx_gpu_SgxNative_readGrouped(
        &g_env, NULL, 1, 1, m, 1, 3, agg, keys ? &k : NULL, starts ? &s : NULL, values ? &v : NULL);
    memcpy(seen8, g_seen, sizeof g_seen);
    if (!r) return -1;
    memcpy(out3, r->data, 24);
    return r->n;
}
