// bcp_scan_host.h -- the host side of the range observation: bcp_range_scan and bcp_final_range_scan over the rows of
// obs_rows() (bcp_ego_host.h), their refusals (the argument checks are scan_check_args of bcp_scan_march.h, which the host
// tests run too), and the one launch of range_scan_kernel (bcp_scan.h).  Included by bcplan.hip after bcp_ego_host.h.
// Capture: the launch arguments depend only on what the caller passes, and nothing is uploaded.  But with a shared map staged
// in LDS the workgroup's dynamic LDS is the mask plus 14 KB of row records, which can pass the 64 KB a kernel gets without
// asking; the first such call on a device raises the function's limit (raise_dynamic_lds: a hipFuncSetAttribute).  So one
// ordinary call with the same maps bound must precede the capture's first call, as for every captured entry point here.
#pragma once

// rec != nullptr: the final states of the episode record, n = capacity, rows j < min(*count, capacity)
static int range_scan(bcp_handle* h, const double* poses, int64_t n, const double* beam_cs, int32_t n_beams, double max_range,
                      float* ranges, int32_t* hit, double* heading_cs_out, void* stream, const EpisodeRec* rec, const char* who)
{
    const double inv_res = h && h->have_map ? h->map.inv_res : 0.0;
    switch (scan_check_args(h != nullptr, beam_cs != nullptr, ranges != nullptr, n_beams, n, h ? h->n : 0, poses != nullptr,
                            rec != nullptr, max_range, inv_res)) {
    case kScanOk: break;
    case kScanNull: return fail(BCP_E_INVALID, "%s: null argument", who);
    case kScanBeams: return fail(BCP_E_INVALID, "%s: n_beams %d outside [1, %d]", who, n_beams, kScanMaxBeams);
    case kScanRows: return fail(BCP_E_INVALID, "%s: n must be positive, and n_envs without poses", who);
    default: return fail(BCP_E_INVALID, "%s: max_range must be finite, > 0 and at most %d cells", who, (int)kScanMaxCells);
    }
    if (!h->have_map) return fail(BCP_E_STATE, "%s: costmaps not set", who);
    if (!poses && !rec && !h->have_state) return fail(BCP_E_STATE, "%s: no poses given and no state bound", who);
    HIP_TRY(hipSetDevice(h->device));
    const ObsRows R = obs_rows(h, rec);
    ScanArgs a;
    memset(&a, 0, sizeof(a));
    a.map = h->map;
    a.valid_rows = h->map_valid_rows;
    a.valid_cols = h->map_valid_cols;
    a.poses = poses;
    const bool delayed = h->params.pose_delay > 0 && R.st.pose_seen;   // the observation shows State.pose, i.e. the delayed pose
    a.sx = delayed ? R.st.pose_seen : R.st.x;
    a.sy = delayed ? R.st.pose_seen + R.n : R.st.y;
    a.sth = delayed ? R.st.pose_seen + 2 * R.n : R.st.angle;
    a.entry = h->n_geoms > 0 ? (R.entry ? R.entry : h->geom_of_env) : R.entry;
    a.live = R.live;
    a.n_envs = R.n;
    a.n = n;
    a.beam_cs = beam_cs;
    a.n_beams = n_beams;
    a.max_range = max_range;
    a.R = max_range * h->map.inv_res;
    a.trip_bound = scan_trip_bound(a.R);
    a.resolution = h->resolution;
    a.ranges = ranges;
    a.hit = hit;
    a.heading_cs = heading_cs_out;
    // One launch.  A workgroup walks 256 rays at a time; with the mask staged in LDS it stays for several such chunks, so that
    // the staging is paid a bounded number of times (2 048 workgroups: eight per CU), otherwise every chunk gets its own.
    const bool staged = h->map.in_lds != 0;
    const int64_t chunks = (n * n_beams + kScanBlock - 1) / kScanBlock;
    const dim3 grid((unsigned)std::min<int64_t>(chunks, staged ? 2048 : (int64_t)1 << 20));
    const void* fn = staged ? (const void*)range_scan_kernel<true> : (const void*)range_scan_kernel<false>;
    return launch_variant(h, fn, grid, dim3(kScanBlock), scan_lds_bytes(h->map), (hipStream_t)stream, a);
}

extern "C" int bcp_range_scan(bcp_handle* h, const double* poses, int64_t n, const double* beam_cs, int32_t n_beams,
                              double max_range, float* ranges, int32_t* hit, double* heading_cs_out, void* stream)
{
    return range_scan(h, poses, n, beam_cs, n_beams, max_range, ranges, hit, heading_cs_out, stream, nullptr, "bcp_range_scan");
}

extern "C" int bcp_final_range_scan(bcp_handle* h, const double* beam_cs, int32_t n_beams, double max_range, float* ranges,
                                    int32_t* hit, double* heading_cs_out, void* stream)
{
    if (h && !h->have_rec) return fail(BCP_E_STATE, "bcp_final_range_scan: no episode record bound");
    return range_scan(h, nullptr, h ? h->rec.capacity : 0, beam_cs, n_beams, max_range, ranges, hit, heading_cs_out, stream,
                      h ? &h->rec : nullptr, "bcp_final_range_scan");
}
