// fusion_ingest.hpp -- how a frame reaches the device ahead of its processFrame call: the host-frame ring with its staging
// thread (mmf_fusion_process_frame_host[_next]) and the next frame's prefetch on the side streams
// (mmf_fusion_prefetch_frame).  Textually included by mmf_hip.hip behind fusion_keypoints.hpp.
#pragma once

static int fusion_process_frame_impl(mmf_fusion* f, const mmf_frame* fr);  // fusion_orchestrator.hpp

// a stream waits for an event only when the event has not happened yet (a wait is a barrier packet on the queue either way)
static hipError_t fusion_wait_unless_done(hipStream_t s, hipEvent_t e) {
    if (hipEventQuery(e) == hipSuccess) return hipSuccess;
    (void)hipGetLastError();
    return hipStreamWaitEvent(s, e, 0);
}

// ---- processFrame(const FrameData&) with the frame still in host memory ------------------------------------------
// The reference uploads FrameData::rgb / depth to GL textures at :221, :261.  Here rgb, depth (and the optional id image)
// go through pinned staging buffers into device copies, three deep, on a stream of their own.
static int fusion_up_init(mmf_fusion* f) {
    if (f->up.pin[0]) return MMF_OK;
    const size_t total = (size_t)f->width * f->height * 8;  // 8 B/px: depth f32, rgb u8 x 3, id u8
    for (int i = 0; i < HostRing::kUp; ++i) {
        MMF_HIP_TRY(f->up.pin[i].create(total));
        MMF_HIP_TRY(f->up.dev[i].create(total));
        MMF_HIP_TRY(f->up.ev[i].create());
        MMF_HIP_TRY(f->up.ev_rgb[i].create());
    }
    MMF_HIP_TRY(f->up.stream.create());
    MMF_HIP_TRY(f->up.begin.create());
    return MMF_OK;
}
// host -> pinned -> device of rgb, then depth, into `slot`, on the upload stream; up.ev_rgb[slot] / up.ev[slot] mark the
// arrivals.  The colour image goes first: the next frame's image side (intensity pyramid, gradients, SO3) needs only that
// and runs beside the chain, the depth side is enqueued behind the pose.  after_begin: see HostRing::host_caught_up.
static int fusion_up_stage(mmf_fusion* f, int slot, const uint8_t* rgb_host, const float* depth_host, bool after_begin,
                           HostRing::Stager* announce) {
    const size_t npix = (size_t)f->width * f->height;
    // the staging buffer's previous upload must have left it (round-2 advisor finding: nothing made sure of that)
    if (f->up.recorded[slot]) MMF_HIP_TRY(hipEventSynchronize(f->up.ev[slot].get()));
    std::memcpy(f->up.pin[slot].get() + npix * 4, rgb_host, npix * 3);
    // the device copy's last readers are frames enqueued before this call (up.begin: recorded when the call began --
    // NOT now: by now this frame's whole tracking chain sits on the fusion's stream and the upload is meant to overlap it)
    if (after_begin) MMF_HIP_TRY(hipStreamWaitEvent(f->up.stream.get(), f->up.begin.get(), 0));
    MMF_HIP_TRY(hipMemcpyAsync(f->up.dev[slot].get() + npix * 4, f->up.pin[slot].get() + npix * 4, npix * 3, hipMemcpyHostToDevice, f->up.stream.get()));
    MMF_HIP_TRY(hipEventRecord(f->up.ev_rgb[slot].get(), f->up.stream.get()));
    if (announce) {
        {
            std::lock_guard<std::mutex> lock(announce->mu);
            announce->rgb_done = true;
        }
        announce->cv.notify_all();
    }
    std::memcpy(f->up.pin[slot].get(), depth_host, npix * 4);
    MMF_HIP_TRY(hipMemcpyAsync(f->up.dev[slot].get(), f->up.pin[slot].get(), npix * 4, hipMemcpyHostToDevice, f->up.stream.get()));
    MMF_HIP_TRY(hipEventRecord(f->up.ev[slot].get(), f->up.stream.get()));
    f->up.recorded[slot] = true;
    return MMF_OK;
}
// the staging thread: one job at a time (HostRing::Stager)
static void fusion_stager_main(mmf_fusion* f) {
    HostRing::Stager& s = f->up.stager;
    (void)hipSetDevice(f->ctx->device);
    std::unique_lock<std::mutex> lock(s.mu);
    for (;;) {
        s.cv.wait(lock, [&] { return s.stop || s.busy; });
        if (s.stop) return;
        const int slot = s.slot;
        const uint8_t* rgb = s.rgb;
        const float* depth = s.depth;
        const bool after_begin = s.after_begin;
        lock.unlock();
        const int rc = fusion_up_stage(f, slot, rgb, depth, after_begin, &s);
        const std::string err = rc ? std::string(mmf_last_error()) : std::string();  // (the error text is per thread)
        lock.lock();
        s.rc = rc, s.error = err, s.busy = false, s.rgb_done = true;
        s.cv.notify_all();
    }
}
// hands the announced frame to the staging thread (started on first use)
static int fusion_stage_host_begin(mmf_fusion* f, bool after_begin) {
    HostRing::HostNext& hn = f->up.next;
    HostRing::Stager& s = f->up.stager;
    if (!s.thread.joinable()) s.thread = std::thread(fusion_stager_main, f);
    {
        std::lock_guard<std::mutex> lock(s.mu);
        s.slot = hn.slot, s.rgb = hn.rgb, s.depth = hn.depth, s.busy = true, s.rgb_done = false, s.after_begin = after_begin;
    }
    s.cv.notify_all();
    hn.pending = true;
    return MMF_OK;
}
// the hinted next frame's upload has been enqueued when this returns (ev_up[slot] recorded): called before anything is told
// to wait for that event -- inside processFrame where the host would only wait for the pose, in the prefetch, or at the
// latest when the call returns
static int fusion_stage_host_next(mmf_fusion* f) {
    HostRing::HostNext& hn = f->up.next;
    if (!hn.pending) return MMF_OK;
    hn.pending = false;
    HostRing::Stager& s = f->up.stager;
    std::unique_lock<std::mutex> lock(s.mu);
    s.cv.wait(lock, [&] { return !s.busy; });
    if (s.rc) return fail(s.rc, s.error);
    hn.staged = hn.rgb_staged = true;
    return MMF_OK;
}
// ... only its colour image's (up.ev_rgb[slot] recorded): what the image side enqueued beside the chain waits for
static int fusion_stage_host_rgb(mmf_fusion* f) {
    HostRing::HostNext& hn = f->up.next;
    if (!hn.pending || hn.rgb_staged) return MMF_OK;
    HostRing::Stager& s = f->up.stager;
    std::unique_lock<std::mutex> lock(s.mu);
    s.cv.wait(lock, [&] { return s.rgb_done; });
    if (!s.busy && s.rc) return MMF_OK;  // (the join reports it)
    hn.rgb_staged = true;
    return MMF_OK;
}

// next_rgb_host / next_depth_host (both or neither): the frame the NEXT call will be given (same pointers, contents
// unchanged until then) -- the host-memory form of mmf_frame::next_*: it is staged and uploaded during this call and its
// sensor-side preparation overlaps this frame's fusion, so the next call starts with its frame on the device.
extern "C" int mmf_fusion_process_frame_host_next(mmf_fusion* f, const uint8_t* rgb_host, const float* depth_host,
                                                  const uint8_t* mask_host, int has_new_label, long long timestamp,
                                                  const float* in_pose, float weight_multiplier, int bootstrap,
                                                  const uint8_t* next_rgb_host, const float* next_depth_host) {
    MMF_REQUIRE(f != nullptr, "mmf_fusion_process_frame_host: null fusion object");
    if (!rgb_host || !depth_host || timestamp < 0) return fail(MMF_ERR_INVALID, "invalid image data");  // :209-212
    mmf_ctx* c = f->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    if (int rc = fusion_up_init(f)) return rc;
    const size_t npix = (size_t)f->width * f->height;
    const size_t o_depth = 0, o_rgb = npix * 4, o_mask = npix * 7;
    HostRing::HostNext& hn = f->up.next;
    if (int rc = fusion_stage_host_next(f)) return rc;  // (nothing of an earlier announcement is still being staged)
    // what a refilled slot's upload has to wait for: the work enqueued before this call -- nothing, when the last call
    // ended with the host holding a pose from the fusion's stream (every lane joins that stream at the end of a frame)
    const bool host_knows = !tunables().host_up_events;
    const bool after_begin = !(host_knows && f->up.host_caught_up);
    if (after_begin) MMF_HIP_TRY(hipEventRecord(f->up.begin.get(), c->stream));
    int slot;
    if (hn.staged && hn.rgb == rgb_host && hn.depth == depth_host) {  // announced by the previous call: already on its way
        slot = hn.slot;
    } else {
        if (hn.staged || hn.pending) f->pre.rgb = nullptr, f->pre.depth = nullptr;  // what was prepared belongs to a frame that never came
        slot = f->up.cur;                                                          // (its device buffer is about to be reused)
        if (int rc = fusion_up_stage(f, slot, rgb_host, depth_host, after_begin, nullptr)) return rc;
    }
    hn = HostRing::HostNext();
    f->up.cur = (slot + 1) % HostRing::kUp;
    // (an announced frame arrived during the last call as a rule: then the fusion's stream gets no barrier packet)
    if (host_knows)
        MMF_HIP_TRY(fusion_wait_unless_done(c->stream, f->up.ev[slot].get()));
    else
        MMF_HIP_TRY(hipStreamWaitEvent(c->stream, f->up.ev[slot].get(), 0));
    mmf_frame fr;
    std::memset(&fr, 0, sizeof(fr));
    fr.rgb = f->up.dev[slot].get() + o_rgb, fr.depth = (const float*)(f->up.dev[slot].get() + o_depth), fr.timestamp = timestamp;
    fr.in_pose = in_pose, fr.weight_multiplier = weight_multiplier, fr.bootstrap = bootstrap;
    fr.icp_refine = 1;
    mmf_segmentation seg;
    std::memset(&seg, 0, sizeof(seg));
    if (mask_host) {  // the id image is this frame's segmentation result: it cannot be announced a frame ahead
        std::memcpy(f->up.pin[slot].get() + o_mask, mask_host, npix);
        MMF_HIP_TRY(hipMemcpyAsync(f->up.dev[slot].get() + o_mask, f->up.pin[slot].get() + o_mask, npix, hipMemcpyHostToDevice, c->stream));
        seg.mask = f->up.dev[slot].get() + o_mask, seg.has_new_label = has_new_label;
        fr.segmentation = &seg;
    }
    if (next_rgb_host && next_depth_host) {
        hn.rgb = next_rgb_host, hn.depth = next_depth_host, hn.slot = f->up.cur;
        fr.next_rgb = f->up.dev[hn.slot].get() + o_rgb, fr.next_depth = (const float*)(f->up.dev[hn.slot].get() + o_depth);
        if (int rc = fusion_stage_host_begin(f, after_begin)) return rc;  // staged and sent up beside this call's own work
    }
    int rc = fusion_process_frame_impl(f, &fr);
    if (rc) {  // the staging thread may still be reading the caller's next_* buffers: not past this call's return
        const std::string why = mmf_last_error();
        (void)fusion_stage_host_next(f);
        return fail(rc, why);
    }
    return fusion_stage_host_next(f);  // (paths that enqueue no prefetch never reached the staging point)
}

extern "C" int mmf_fusion_process_frame_host(mmf_fusion* f, const uint8_t* rgb_host, const float* depth_host,
                                             const uint8_t* mask_host, int has_new_label, long long timestamp,
                                             const float* in_pose, float weight_multiplier, int bootstrap) {
    return mmf_fusion_process_frame_host_next(f, rgb_host, depth_host, mask_host, has_new_label, timestamp, in_pose,
                                              weight_multiplier, bootstrap, nullptr, nullptr);
}

// The filter and the input-side preparation (vertex / normal maps, depth and intensity pyramids, gradients) of the
// NEXT frame, enqueued on a second stream so that they run while the current frame is still being fused.
// rgb / depth must stay unchanged until the mmf_fusion_process_frame call that consumes them (same pointers).
// `tick_at_use`: the tick of the processFrame call these buffers are for
static int fusion_prefetch_init(mmf_fusion* f) {
    if (f->pre.side) return MMF_OK;
    MMF_HIP_TRY(f->pre.side.create());
    MMF_HIP_TRY(f->pre.side2.create());
    MMF_HIP_TRY(f->pre.done.create());
    MMF_HIP_TRY(f->pre.done2.create());
    MMF_HIP_TRY(f->pre.partials.create((size_t)kMaxGrid * kPartialStride));
    MMF_HIP_TRY(f->pre.ticket.create(kTicketWords));
    MMF_HIP_TRY(hipMemsetAsync(f->pre.ticket.get(), 0, sizeof(unsigned) * kTicketWords, f->pre.side2.get()));
    MMF_HIP_TRY(f->pre.so3_mem.create(2));
    f->pre.so3_stage[0] = f->pre.so3_mem.get(), f->pre.so3_stage[1] = f->pre.so3_stage[0] + 1;
    MMF_HIP_TRY(hipMemsetAsync(f->pre.so3_stage[0], 0, 2 * sizeof(OdomState), f->pre.side2.get()));
    return MMF_OK;
}

// The image side of the frame the call with tick `tick_at_use` will be given: intensity pyramid + gradients into the
// free halves of their double buffers, then the SO3 pre-alignment (this frame's against the last frame's level-2 image:
// no model, no pose) in the staging state of that tick's parity.  Second side stream; needs the streams to exist.
// ahead: enqueued at the start of a frame whose own image side was prepared on this same stream (nothing to wait for);
// else behind ev_inputs_free where a frame recorded it (the first frame's intensity pyramid and an untracked frame's
// preparation are written on the fusion's stream; after a tracked frame the host has the poses: everything is done)
static int fusion_prefetch_image(mmf_fusion* f, const uint8_t* rgb, int tick_at_use, bool ahead) {
    const mmf_fusion_config& g = f->cfg;
    mmf_odom* odom = f->models[0]->odom;
    hipStream_t img_stream = f->pre.side2.get();
    if (!ahead && f->pre.inputs_free_recorded) MMF_HIP_TRY(hipStreamWaitEvent(img_stream, f->pre.inputs_free.get(), 0));
    Enqueuer qi(img_stream);
    PrepSensorFrame sf;
    sf.rgb = rgb, sf.channels = 3;
    int rc = odom_prepare_sensor(odom, sf, PREP_INPUT_IMAGE, &qi);
    if (rc) return rc;
    f->pre.so3_ready = -1;
    if (g.so3 && tick_at_use > 1) {  // a model exists: the frame will be tracked, SO3 first
        const int s = tick_at_use & 1;
        rc = odom_prefetch_so3(odom, qi, f->pre.partials.get(), f->pre.ticket.get(), f->pre.so3_stage[s]);
        if (rc) return rc;
        f->pre.so3_ready = s;
    }
    MMF_HIP_TRY(qi.flush());
    MMF_HIP_TRY(hipEventRecord(f->pre.done2.get(), img_stream));
    f->pre.image_rgb = rgb;
    return MMF_OK;
}

static int fusion_prefetch_impl(mmf_fusion* f, const uint8_t* rgb, const float* depth, int tick_at_use) {
    mmf_ctx* c = f->ctx;
    MMF_HIP_TRY(hipSetDevice(c->device));
    mmf_odom* odom = f->models[0]->odom;
    if (int rc0 = fusion_prefetch_init(f)) return rc0;
    f->pre.valid = false;  // an earlier prefetch is simply overwritten: same streams, same order
    if (f->up.next.slot >= 0 && f->up.dev[0].get() && rgb == f->up.dev[f->up.next.slot].get() + (size_t)f->width * f->height * 4) {
        // the hinted frame comes from host memory (mmf_fusion_process_frame_host_next): behind its upload
        if (int rc0 = fusion_stage_host_next(f)) return rc0;
        if (hipEventQuery(f->up.ev[f->up.next.slot].get()) != hipSuccess) {  // (as a rule it arrived long ago: no barrier packets)
            (void)hipGetLastError();
            MMF_HIP_TRY(hipStreamWaitEvent(f->pre.side.get(), f->up.ev[f->up.next.slot].get(), 0));
            MMF_HIP_TRY(hipStreamWaitEvent(f->pre.side2.get(), f->up.ev[f->up.next.slot].get(), 0));
        }
    }
    if (f->pre.inputs_free_recorded) MMF_HIP_TRY(hipStreamWaitEvent(f->pre.side.get(), f->pre.inputs_free.get(), 0));
    const mmf_fusion_config& g = f->cfg;
    // depth chain (first side stream): filter, depth pyramid, vertex and normal maps -- what the chains' ICP term reads,
    // hence behind ev_inputs_free.  Enqueued before the image chain when that is still to come: it is five launches that
    // start with the 40 us filter, the image chain fifteen short ones.
    float* target = f->pre.filtered[1 - f->pre.cur].get();
    Enqueuer qd(f->pre.side.get());
    int rc = filter_depth_on(c, qd, depth, f->width, f->height, g.depth_cutoff, target);
    if (rc) return rc;
    PrepSensorFrame sf;
    sf.depth_filtered = target, sf.depth_cutoff = g.max_depth_processed;
    rc = odom_prepare_sensor(odom, sf, PREP_INPUT_DEPTH, &qd);
    if (rc) return rc;
    MMF_HIP_TRY(qd.flush());
    if (f->pre.image_rgb != rgb) {  // (else: enqueued at the start of the frame)
        rc = fusion_prefetch_image(f, rgb, tick_at_use, false);
        if (rc) return rc;
    }
    // ONE event for the consumer: the first side stream takes in the second's (one wait less on the model's stream)
    MMF_HIP_TRY(hipStreamWaitEvent(f->pre.side.get(), f->pre.done2.get(), 0));
    MMF_HIP_TRY(hipEventRecord(f->pre.done.get(), f->pre.side.get()));
    f->pre.valid = true, f->pre.rgb = rgb, f->pre.depth = depth;
    return MMF_OK;
}

extern "C" int mmf_fusion_prefetch_frame(mmf_fusion* f, const uint8_t* rgb, const float* depth) {
    MMF_REQUIRE(f && rgb && depth, "mmf_fusion_prefetch_frame: null argument");
    return fusion_prefetch_impl(f, rgb, depth, f->tick);
}
