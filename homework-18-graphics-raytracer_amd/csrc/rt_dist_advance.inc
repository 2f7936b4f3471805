/* rt_dist_advance.inc — one step of the scatter chain after its cast (distributed_ray_trace, main.rs:521-614, with
 * get_refract's loop, main.rs:343-405, unrolled into one cast per step).  Textually included in the body of the chain
 * kernel (rt_dist_kernels.h), which defines the names it uses:
 *   in/out  phase, req, h, h_in_dir, h_in_mode, sdir, kind, sp, travel, retry, rng
 *   in      cr (the cast's result), sc, fr, dp, epoch, out_index, n_pixels, n_samples, emit_request(view)
 *   out     casting (another cast is due: phase and req say which), terminal (the sample ends in a get_shade request)
 * Every random draw of a level is made here, in the reference's order. */
        enum { GO_LEVEL, GO_TRY_EXIT, GO_END } go = GO_END;
        bool terminal = false; /* the sample's value is a get_shade (request slot sp); else black */
        HitGeom ih = h;
        if (cr.prim >= 0) ih = finish_hit(sc, req, cr, false); /* the hit just found */
        V3 i_in_dir = req.d;
        uint32_t i_in_mode = req.mode;

        if (phase == DP_PRIMARY) {
            if (cr.prim >= 0) { /* a miss: black (main.rs:1154) */
                h = ih;
                h_in_dir = req.d;
                h_in_mode = req.mode;
                go = GO_LEVEL;
            }
        } else if (phase == DP_NEXT) {
            if (cr.prim < 0) {
                if (kind != 2u) { /* get_shade(&scattered_hit): the same hit seen along the scattered direction (main.rs:573, 592) */
                    emit_request(sdir);
                    terminal = true;
                } /* kind 2: black (main.rs:606-608) */
            } else {
                /* the level's factor, before `h` moves on to the next hit (main.rs:566-570, 585-589, 605) */
                V3 factor;
                if (kind == 2u) {
                    factor = v3(rtdm::powf(sc.materials[h.obj].opaque_decay, travel), 0.0f, 0.0f);
                } else {
                    const Mat m = material_approx(sc.materials[h.obj], h.u, h.v);
                    const V3 view = -h_in_dir;
                    factor = kind == 0u ? get_diffuse(m, h.normal, req.d) : get_specular(m, h.normal, view, req.d);
                }
                dp.sp_frame[(size_t)sp * n_samples + (size_t)epoch * n_pixels + out_index] = make_float4(factor.x, factor.y, factor.z, duf(kind));
                h = ih;
                h_in_dir = req.d;
                h_in_mode = req.mode;
                emit_request(req.d); /* get_shade(&next_hit) (main.rs:565, 584, 604): frame sp's shade */
                sp += 1;
                go = GO_LEVEL;
            }
        } else { /* DP_REFR_INSIDE / DP_REFR_BOUNCE; a miss is Refraction::Infinite -> black (main.rs:610) */
            if (cr.prim >= 0) {
                if (phase == DP_REFR_INSIDE) {
                    travel = distance(ih.pos, h.pos);
                    retry = 0;
                } else {
                    travel += distance(req.o, ih.pos);
                    retry += 1;
                }
                go = GO_TRY_EXIT;
            }
        }

#ifdef RT_STEP_TICK
        RT_STEP_TICK(10)
#endif
        bool casting = false;
        if (go == GO_LEVEL) {
            /* distributed_ray_trace(state, &h), depth = max_depth - sp */
            const int32_t depth = fr.max_depth - sp;
            if (depth <= 0) { /* main.rs:524-527: get_shade(&hit) */
                emit_request(h_in_dir);
                terminal = true;
            } else {
                const rt_material &rm = sc.materials[h.obj];
                /* weighted_select (main.rs:652-666) */
                const float w0 = (1.0f - rm.shiness) * (1.0f - rm.transparency);
                const float w1 = rm.shiness * (1.0f - rm.transparency);
                const float w2 = rm.transparency;
                float wsum = 0.0f;
                wsum = wsum + w0;
                wsum = wsum + w1;
                wsum = wsum + w2;
                uint32_t word_sel, word_phi, word_theta; /* the level's three draws, in stream order */
                next_u32x3(rng, &word_sel, &word_phi, &word_theta);
                const float rsel = range_f32_of(word_sel, 0.0f, wsum);
                float acc = 0.0f;
                acc += w0;
                kind = 2u;
                if (rsel < acc) kind = 0u;
                else {
                    acc += w1;
                    if (rsel < acc) kind = 1u;
                }
                /* scatter_hit (main.rs:539-554) */
                const float exponent = kind == 0u ? 1.0f : rm.smoothness;
                const V3 lobe = kind == 0u ? -h.normal : h_in_dir;
                const float phi = rtdm::acosf(rtdm::powf(1.0f - range_f32_of(word_phi, 0.0f, 1.0f), exponent));
                const float theta = range_f32_of(word_theta, -RT_F_PI, RT_F_PI);
                float sphi, cphi, stheta, ctheta;
                rtdm::sincosf(phi, &sphi, &cphi);
                rtdm::sincosf(theta, &stheta, &ctheta);
                sdir = adjust_normal(v3(sphi * ctheta, sphi * stheta, cphi), normalize(lobe));
                const float cosine = -dot(h.normal, sdir);
                if (!(cosine <= 0.0f)) { /* else black (main.rs:560, 579, 598) */
                    if (kind != 2u) { /* get_reflect(&scattered_hit) (main.rs:328-341) */
                        req.o = h.pos;
                        req.d = reflect_dir(h.normal, sdir);
                        req.mode = h_in_mode;
                        req.excl = pack_excl(h.prim, h.bf ? FACE_FRONT : FACE_BACK);
                        phase = DP_NEXT;
                        casting = true;
                    } else { /* get_refract(&scattered_hit, 100.0) (main.rs:343-405); Trapped -> black */
                        V3 refract_in;
                        if (refract_dir(h.normal, sdir, rm.refraction_index, &refract_in)) {
                            req.o = h.pos;
                            req.d = normalize(refract_in);
                            req.mode = FACE_BACK;
                            req.excl = pack_excl(h.prim, FACE_FRONT);
                            phase = DP_REFR_INSIDE;
                            casting = true;
                        }
                    }
                }
            }
        } else if (go == GO_TRY_EXIT) {
            const rt_material &rm = sc.materials[h.obj];
            V3 out_dir;
            const bool have_out = refract_dir(ih.normal, i_in_dir, 1.0f / rm.refraction_index, &out_dir);
            if (!have_out && travel <= 100.0f && retry < 10) {
                req.o = ih.pos;
                req.d = reflect_dir(ih.normal, i_in_dir);
                req.mode = i_in_mode;
                req.excl = pack_excl(ih.prim, ih.bf ? FACE_FRONT : FACE_BACK);
                phase = DP_REFR_BOUNCE;
                casting = true;
            } else if (have_out) { /* escape ray, main.rs:393-401; else Trapped -> black */
                req.o = ih.pos;
                req.d = normalize(out_dir);
                req.mode = FACE_FRONT;
                req.excl = pack_excl(ih.prim, FACE_BACK);
                phase = DP_NEXT;
                casting = true;
            }
        }
#ifdef RT_STEP_TICK
        RT_STEP_TICK(12)
#endif
