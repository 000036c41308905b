// The fused operand prologue of dy on the four floats of piece r of a chunk: o[0..3] = act(c1 x1 + c2 x2 + c0), zero from flat index
// `valid` on (frames past T: the prologue's constant must not leak into them, and what a piece read past its row must not either).
// A FRAGMENT like the kernel bodies (ctrgc_stream_body.h), pasted where p1[i], p2[i], c1, c2, c0, dy, r and valid are in scope.
                float o[4] = {fmaf(c1, p1[i].x, fmaf(c2, p2[i].x, c0)), fmaf(c1, p1[i].y, fmaf(c2, p2[i].y, c0)),
                              fmaf(c1, p1[i].z, fmaf(c2, p2[i].z, c0)), fmaf(c1, p1[i].w, fmaf(c2, p2[i].w, c0))};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (dy.act == 1) o[k] = fmaxf(o[k], 0.f);
                    if (r * 4 + k >= valid) o[k] = 0.f;
                }
