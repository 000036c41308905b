"""Audit of the read slack behind the tensors the 16-byte kernels stream ("Read slack behind streamed activations").

At joint counts V that are not a multiple of 4 some kernels read the last 16-byte piece of a frame whole: up to 12 bytes past
the last element of a source activation.  include/tamgcn.h asks for 16 readable bytes behind such a buffer; the library sees
pointers only, so the obligation is the Python layer's (ops.empty allocates ops.SLACK floats extra, ops.with_slack copies a
tensor that ends with its storage).  Two parts, test-side only:

  CLASSES        every device pointer the binding passes as `const float*` -- each struct field and each entry-point parameter
                 stream_audit.parse_header() yields as kind 'r', tamgcn_src.x1 / x2 / coef once per field that holds a tamgcn_src
                 -- has exactly one class:
                   stream    read in 16-byte pieces from rows that may be only dword aligned: needs 16 readable bytes behind the
                             tensor's last element whenever the launch's row length V is not a multiple of 4 (Entry.v says
                             where that V comes from);
                   guarded   the kernel never reads past the last element (Entry.cites: csrc file and literal text of the guard);
                   flat      not an activation, or indexed element by element (Entry.why).
                 Written from the header's statements and from reading the kernels, not from a measurement.
  SlackAuditor   a context manager over stream_audit.LibraryTap: before every library launch, for every `stream` pointer of a
                 ragged launch, it resolves the address to the tensor that holds it and requires storage_end - tensor_end >= 16
                 on the torch storage, exactly as ops.with_slack measures it; a violation raises SlackError WITHOUT calling
                 into the library.
"""
import os
import sys

import stream_audit as A

CSRC = os.path.join(A.ROOT, 'tam_gcn_amd', 'csrc')
SLACK_BYTES = 16
STREAM, GUARDED, FLAT = 'stream', 'guarded', 'flat'


class Entry:
    """cls; v: where the row length of a launch comes from -- 'desc' (field V of the descriptor that holds the pointer), 'arg:V'
    (the entry point's parameter V) or 'arg:<name>' (field V of the descriptor passed as parameter <name>); cites: [(csrc file,
    literal text)]; why: one line."""
    __slots__ = ('cls', 'v', 'cites', 'why')

    def __init__(self, cls, v=None, cites=(), why=''):
        self.cls, self.v, self.cites, self.why = cls, v, tuple(cites), why


def stream(v, why):
    return Entry(STREAM, v=v, why=why)


def guarded(*cites, why=''):
    return Entry(GUARDED, cites=cites, why=why)


def flat(why):
    return Entry(FLAT, why=why)


# ---- the guards, named once -------------------------------------------------------------------------------------------
G_ROW = ('rowwise.h', 'plus a scalar tail of L % 4 elements')
G_ROW_TAIL = ('elementwise.hip', 'for (int i = (L & ~3) + li; i < L; i += geo.tpr)')
G_DROP_TAIL = ('dropout.hip', 'for (int i = (L & ~3) + li; i < L; i += geo.tpr)')
G_SRC_VALUE = ('elementwise.hip', 'src_value(src, ')
G_POOL_BWD = ('elementwise.hip', 'if (start >= 0 && start + 4 <= L)')
G_CONV_EPI = ('conv.hip', 'if ((vecok || v + 4 <= Vs) && col + 4 <= ncols)')
G_WGRAD_SLOT = ('wgrad.hip', 'if (va && vb) o = *reinterpret_cast<const float4*>(p);')
G_WGRAD_TAIL = ('wgrad.hip', 'const int po = pc < cpf ? pc * W_PC : wlen - W_PC;')
G_FUSED_V20 = ('ctrgc.hip', 'if (d->V != 20 || (d->S != 1 && d->S != 3))')
G_DE_ACC = ('ctrgc_de.hip', 'static constexpr bool VEC = (V % 4 == 0);')
G_DE_TAIL = ('ctrgc_de.hip', 'pre[i] = e < 16 * VV / 4 ? g[e] : make_float4(0.f, 0.f, 0.f, 0.f);')
G_DE_TAIL_DMA = ('ctrgc_de.hip', 'lanes past the chunk re-read its last slot into the padding')
G_TILED_V = ('ctrgc_tiled.hip', 'TG_CHECK(tiled_v_ok(d->V), "tamgcn_ctrgc_tiled_de_tail')
G_VGEN_TAIL = ('vgen.hip', 'w0 + col < VV ? dEg[(long long)sc * VV + w0 + col] : 0.f')
G_E_TILED = ('ctrgc_stream_body.h', 't[i] = Eg[(((long long)n * ST + s) * Cout + c) * VV + r];')
G_E_VGEN = ('ctrgc_stream_body.h', 't[i] = g[e < VV ? e : 0];')
G_F2_PADDED = ('f2x_body.h', 'PADDED: the source has frames of VP floats')
G_F2S = ('f2s_common.h', 'return fs_keep(p[ok ? i : 0], ok);')
G_STEM = ('stemhead.hip', 'x[xb + i]')
G_SAL = ('saliency.hip', 'dx0[((((long long)n * M + m) * C + c) * T + t) * V + v]')
G_GUIDE_RGB = ('guidance.hip', 'const int nv = (W - head) >> 2, tail = head + 4 * nv;')
G_CLIP_EXTENT = ('clipfeeder.hip', 'const bool vec = ((long long)T * V * M) % 4 == 0')
G_CLIP_ROW = ('clipfeeder.hip', 'const bool vec = rowlen % 4 == 0')
G_CLIP_SPAN = ('clipfeeder.hip', 'if (i >= ilo && i + VEC <= ihi)')
G_RING = ('streaming.hip', 'const bool vec = VM % 4 == 0 && aligned16(ring) && aligned16(out);')
G_TCONV_MASK = ('tconv.hip', 'if (col0 + 4 > ncols) col0 = 0;')

W_COEF = 'per-channel prologue coefficients [3][ctot]'
W_WEIGHT = 'weights'
W_BIAS = 'per-channel vector'
W_PART = 'partial sums, indexed element by element'
W_SAVE = 'per-channel saved statistics'
W_SCORES = '(N, K) scores or logits, indexed element by element'

CLASSES = {}


def _put(owner, **fields):
    for name, e in fields.items():
        key = (owner, name.replace('__', '.'))
        assert key not in CLASSES, key
        CLASSES[key] = e


def _src(owner, field, x1, x2=None):
    """The three pointers of a tamgcn_src held by `owner` as `field`."""
    _put(owner, **{field + '__x1': x1, field + '__x2': x2 if x2 is not None else x1, field + '__coef': flat(W_COEF)})


# ---- GEMMs ------------------------------------------------------------------------------------------------------------
_S_CONV = stream('desc', 'conv.hip stages frames of Vp = V rounded up to 4 floats: the last piece of a frame is read whole')
_src('tamgcn_conv_desc', 'src', _S_CONV)
_src('tamgcn_conv_desc', 'mask', guarded(G_CONV_EPI, why='epilogue operand: whole groups of four valid columns, else per element'))
_put('tamgcn_conv_desc', w=flat(W_WEIGHT), bias=flat(W_BIAS), bcast=flat('[M][N][V], indexed per joint'),
     add1=guarded(G_CONV_EPI), add2=guarded(G_CONV_EPI), aux=guarded(G_CONV_EPI), aux_center=flat(W_SAVE), post_coef=flat(W_COEF))
_src('tamgcn_conv_pair_desc', 'src', stream('desc', 'the LDS-DMA form of conv.hip; ops.pair_supported admits V % 4 == 0 only'))
_put('tamgcn_conv_pair_desc', w0=flat(W_WEIGHT), w1=flat(W_WEIGHT), bias0=flat(W_BIAS), bias1=flat(W_BIAS))
_G_WGRAD = guarded(G_WGRAD_SLOT, G_WGRAD_TAIL, why='a slot cut by the end of a row is loaded per element; the last chunk is re-fetched from [len - 32, len)')
_src('tamgcn_wgrad_desc', 'gy', _G_WGRAD)
_src('tamgcn_wgrad_desc', 'src', _G_WGRAD)
for _f in ('gy0', 'gy1', 'src'):
    _src('tamgcn_wgrad_pair_desc', _f, _G_WGRAD)
_put('tamgcn_reduce_desc', part=flat(W_PART))

# ---- BatchNorm bookkeeping ---------------------------------------------------------------------------------------------
for _o in ('tamgcn_bn_fwd_desc', 'tamgcn_bn_fwd_finalize'):
    _put(_o, part=flat(W_PART), gamma=flat(W_BIAS), beta=flat(W_BIAS))
for _o in ('tamgcn_bn_bwd_desc', 'tamgcn_bn_bwd_finalize'):
    _put(_o, part=flat(W_PART), gamma=flat(W_BIAS), save=flat(W_SAVE))
_put('tamgcn_coef_diff', coef_d=flat(W_COEF), coef_y=flat(W_COEF))

# ---- CTRGC -------------------------------------------------------------------------------------------------------------
_G_FUSED = guarded(G_FUSED_V20, why='read by the fused V = 20 kernels only: another V is refused before any launch')
_src('tamgcn_ctrgc_desc', 'x', _G_FUSED)
_put('tamgcn_ctrgc_desc', pq=flat('E-builder parameter [S*2*R][N][V], indexed per element'), w3=flat(W_WEIGHT), b3=flat(W_BIAS),
     w4=flat(W_WEIGHT), b4=flat(W_BIAS), A=flat('E-builder parameter [S][V][V]'), alpha=flat('device scalar'), E=_G_FUSED)
_src('tamgcn_ctrgc_bwd_dx3', 'dy', _G_FUSED)
_G_ACC = guarded(G_DE_ACC, why='16-byte loads only in the V % 4 == 0 instantiation')
_src('tamgcn_ctrgc_bwd_de_acc', 'dy', _G_ACC)
_put('tamgcn_ctrgc_bwd_de_acc', x3=_G_ACC)
_put('tamgcn_ctrgc_bwd_de_tail', dE=guarded(G_DE_TAIL, G_DE_TAIL_DMA, why='a 16-channel chunk of V*V floats is a multiple of 4 floats and bounded'))
_put('tamgcn_ctrgc_tiled_de_tail', dE=guarded(G_TILED_V, why='V in {32, 64} only'))
_put('tamgcn_vgen_de_tail', dE=guarded(G_VGEN_TAIL, why='element loads under a bound'))
_S_X3 = 'ctrgc_stream_body.h: chunks of 32 frames in 16-byte pieces from dword-aligned rows; cut4 zeroes what lies past the chunk'
for _fam, _ge in (('tamgcn_ctrgc_tiled_', G_E_TILED), ('tamgcn_vgen_', G_E_VGEN)):
    _put(_fam + 'agg_fwd', x3=stream('arg:d', _S_X3), E=guarded(_ge, why='stage_E: element loads unless V % 4 == 0 is known'))
    _src(_fam + 'agg_bwd', 'dy', stream('arg:d', _S_X3))
    _put(_fam + 'agg_bwd', E=guarded(_ge, why='stage_E: element loads unless V % 4 == 0 is known'))
    _src(_fam + 'de_acc', 'dy', stream('arg:d', _S_X3))
    _put(_fam + 'de_acc', x3=stream('arg:d', _S_X3))

# ---- row-wise element-wise kernels -------------------------------------------------------------------------------------
_G_ROWS = guarded(G_ROW, G_ROW_TAIL, why='L / 4 groups of four inside the row, then a scalar tail')
_G_VAL = guarded(G_SRC_VALUE, why='one element per access through src_value()')
_src('tamgcn_tmean', 'src', _G_VAL)
for _o in ('tamgcn_gcn_tail_fwd', 'tamgcn_gcn_tail_fwd_bits'):
    for _f in ('y', 'o', 'res'):
        _src(_o, _f, _G_ROWS)
_src('tamgcn_gcn_tail_bwd', 'o', _G_ROWS)
_put('tamgcn_gcn_tail_bwd', dg=_G_ROWS, g=_G_ROWS, o_save=flat(W_SAVE))
_src('tamgcn_gcn_tail_bwd_bits', 'o', _G_ROWS)
_put('tamgcn_gcn_tail_bwd_bits', dg=_G_ROWS, o_save=flat(W_SAVE))
_put('tamgcn_gcn_mid_bwd', dsum=_G_ROWS, ddiff=_G_ROWS, y_pre=_G_ROWS, y_save=flat(W_SAVE), r_pre=_G_ROWS, r_save=flat(W_SAVE))
_src('tamgcn_maxpool_fwd', 'src', _G_VAL)
_src('tamgcn_maxpool_post_fwd', 'src', _G_VAL)
_put('tamgcn_maxpool_post_fwd', coef=flat(W_COEF), add=guarded(('elementwise.hip', 'if (add) o += add[yb + i];')))
_G_PB = guarded(G_POOL_BWD, G_SRC_VALUE, why='a group that sticks out of the row is fetched element by element')
_src('tamgcn_maxpool_bwd', 'gy', _G_PB)
_src('tamgcn_maxpool_bwd', 'src', _G_PB)
_put('tamgcn_maxpool_bwd', src_save=flat(W_SAVE))
for _o in ('tamgcn_add_act_fwd', 'tamgcn_add_act_fwd_bits'):
    for _f in ('a', 'res'):
        _src(_o, _f, _G_ROWS)
_put('tamgcn_add_act_bwd', dout=_G_ROWS, out=_G_ROWS, a_pre=_G_ROWS, a_save=flat(W_SAVE), r_pre=_G_ROWS, r_save=flat(W_SAVE))
_put('tamgcn_add_act_bwd_bits', dout=_G_ROWS, a_pre=_G_ROWS, a_save=flat(W_SAVE), r_pre=_G_ROWS, r_save=flat(W_SAVE))
_G_DROP = guarded(G_ROW, G_DROP_TAIL, why='L / 4 groups of four inside the row, then a scalar tail')
for _f in ('a', 'res'):
    _src('tamgcn_drop_add_act_fwd', _f, _G_DROP)
_put('tamgcn_drop_add_act_bwd', dout=_G_DROP, a_pre=_G_DROP, a_save=flat(W_SAVE), r_pre=_G_DROP, r_save=flat(W_SAVE))
_src('tamgcn_apply', 'src', _G_VAL)

# ---- MS-TCN second stage -----------------------------------------------------------------------------------------------
_src('tamgcn_tconv_desc', 'src', stream('desc', 'tconv.hip line buffer: pieces of frames of Vp = V rounded up to 4 floats (forward, backward)'))
_put('tamgcn_tconv_desc', mask__x1=stream('desc', 'the weight gradient stages the forward source in Vp pieces; the backward reads it under ' + G_TCONV_MASK[1]),
     mask__x2=flat('never read: the mask operand has one source'), mask__coef=flat(W_COEF),
     w=flat(W_WEIGHT), bias=flat(W_BIAS), center=flat(W_SAVE))

# ---- stem, head, loss, scores ------------------------------------------------------------------------------------------
_G_STEM = guarded(G_STEM, why='stemhead.hip indexes every activation element by element')
_put('tamgcn_stem_stats', x=guarded(('stemhead.hip', 'bb[k] = xp[(long long)(t + k) * VM];')), dout=guarded(('stemhead.hip', 'aa[k] = dp ? dp[(long long)(t + k) * V] : bb[k];')), center=flat(W_SAVE))
_put('tamgcn_stem_apply', x=_G_STEM, dout=guarded(('stemhead.hip', 'dout[o]')), coef=flat(W_COEF))
_put('tamgcn_head_pool_fwd', x=guarded(('stemhead.hip', 'for (int i = lane; i < L; i += 64) s += p[i];'), why='one wave per row, element loads'))
_put('tamgcn_head_pool_bwd', dpooled=flat('(N, C), one element per row'))
_put('tamgcn_head_fc_fwd', pooled=flat('(N, C) features'), W=flat(W_WEIGHT), b=flat(W_BIAS))
_put('tamgcn_head_fc_bwd', dlogits=flat(W_SCORES), pooled=flat('(N, C) features'), W=flat(W_WEIGHT))
_put('tamgcn_head_fc_grouped', pooled=flat('(G*N, C) features'), W=flat(W_WEIGHT), b=flat(W_BIAS))
_put('tamgcn_stem_streams_eval', x=guarded(('stemhead.hip', 'const float cur = xr[vm];'), why='one element per thread; the frame after the last is never read'), coef=flat(W_COEF))
_put('tamgcn_ce_desc', logits=flat(W_SCORES), probs=flat(W_SCORES), weight=flat('(K) class weights'))
_put('tamgcn_ce_fwd', logits=flat(W_SCORES))
_put('tamgcn_ce_bwd', g=flat(W_SCORES), dloss=flat('device scalar'))
_put('tamgcn_ce_opts_bwd_rows', g=flat(W_SCORES), dloss=flat('(N) row losses'))
_put('tamgcn_score_fuse', scores=flat(W_SCORES), weights=flat('(S) stream weights'))
_put('tamgcn_eval_accumulate', logits=flat(W_SCORES))
_put('tamgcn_score_sweep', a=flat(W_SCORES), b=flat(W_SCORES), alphas=flat('host array'))
_put('tamgcn_window_vote', logits=flat(W_SCORES))
_put('tamgcn_score_ema', probs=flat(W_SCORES))
_put('tamgcn_bank_ema', probs=flat(W_SCORES))
_put('tamgcn_bank_decide', conf=flat('(S) confidences'))
_put('tamgcn_optim_desc', g=flat('flat gradient bucket, 16-byte aligned and n-bounded'), lr=flat('device scalar'))

# ---- input side --------------------------------------------------------------------------------------------------------
_put('tamgcn_stream_derive', x=guarded(('feeder.hip', 'if (e >= total) return;'), why='one element per thread'))
_put('tamgcn_clip_extent', raw=guarded(G_CLIP_EXTENT, why='16-byte form only for planes of whole groups of four'))
_put('tamgcn_clip_transform', raw=guarded(G_CLIP_ROW, G_CLIP_SPAN))
_put('tamgcn_clip_resize', raw=guarded(G_CLIP_ROW), rot=flat('[B][9] rotation matrices'))
_put('tamgcn_window_clip', ring=guarded(G_RING))
_put('tamgcn_bank_window_clip', ring=guarded(G_RING))

# ---- small-batch eval families -----------------------------------------------------------------------------------------
_S_F2X = 'f2x_body.h f2x_stage<PADDED = false>: the last piece of a frame of the contiguous block input reaches VP - V floats past it'
_put('tamgcn_f2_gcn_desc', x=stream('desc', _S_F2X), xpart=guarded(G_F2_PADDED),
     w12=flat(W_WEIGHT), b12=flat(W_BIAS), w4=flat(W_WEIGHT), b4=flat(W_BIAS), A=flat('[S][V][V]'), alpha=flat('device scalar'),
     w3=flat(W_WEIGHT), b3=flat(W_BIAS), sy=flat(W_BIAS), ty=flat(W_BIAS), wd=flat(W_WEIGHT), bd=flat(W_BIAS))
_put('tamgcn_f2_gemm_desc', x=guarded(G_F2_PADDED), add=guarded(G_F2_PADDED), w=flat(W_WEIGHT), b=flat(W_BIAS))
_put('tamgcn_f2_tcn_desc', h=guarded(G_F2_PADDED), x=stream('desc', _S_F2X), wt=flat(W_WEIGHT), bt=flat(W_BIAS), sp=flat(W_BIAS),
     tp=flat(W_BIAS), wr=flat(W_WEIGHT), br=flat(W_BIAS))
_G_F2S = guarded(G_F2S, why='activations are loaded element by element; only 16-byte aligned weights take 16-byte loads')
_put('tamgcn_f2s_gcn_desc', x=_G_F2S, Ae=flat('[K][V][V]'), wg=flat(W_WEIGHT), bg=flat('[Cout][V] bias table'))
_put('tamgcn_f2s_tcn_desc', h=_G_F2S, x=_G_F2S, wt=flat(W_WEIGHT), bt=flat(W_BIAS), wr=flat(W_WEIGHT), br=flat(W_BIAS))
_put('tamgcn_f2s_tcn_bwd_desc', gout=_G_F2S, out=_G_F2S, h=_G_F2S, wtb=flat(W_WEIGHT))
_put('tamgcn_f2s_gcn_bwd_desc', dh=_G_F2S, gout=_G_F2S, out=_G_F2S, Ae=flat('[K][V][V]'), wgb=flat(W_WEIGHT), wrb=flat(W_WEIGHT))

# ---- saliency, guidance ------------------------------------------------------------------------------------------------
_put('tamgcn_saliency_joints', dx0=guarded(G_SAL), coef=flat(W_COEF))
_put('tamgcn_saliency_accumulate', sal=flat('(N, V) joint saliency, indexed per element'))
_put('tamgcn_guidance_reduce', h=guarded(('guidance.hip', 'const float* src = h + (long long)row * C * P + (ok ? p : 0);'), why='one element per lane, clamped to the row'))
_put('tamgcn_guidance_weights', intensity=flat('(N, T\', V, M), indexed per element'), minmax=flat('[parts][2]'))
_put('tamgcn_guidance_apply', weights=flat('(N, J)'), rgb=guarded(G_GUIDE_RGB, why='scalar head and tail around the aligned groups of a row'))


# =====================================================================================================================
# the binding against the table
# =====================================================================================================================
def float_read_pointers(structs=None, funcs=None):
    """[(owner, name)]: every `const float*` of the header -- struct fields by struct, parameters by entry point; a tamgcn_src
    (by value, or behind a pointer) counts as name.x1, name.x2 and name.coef of the field or parameter that holds it."""
    if structs is None:
        structs, funcs = A.parse_header()
    out = []
    for owner, decls in list(structs.items()) + list(funcs.items()):
        if owner == 'tamgcn_src':
            continue
        for d in decls:
            if d.kind == 'r' and d.base == 'float':
                out.append((owner, d.name))
            elif d.kind in ('struct', 'desc') and d.base == 'tamgcn_src':
                out += [(owner, f'{d.name}.{f.name}') for f in structs['tamgcn_src'] if f.kind == 'r' and f.base == 'float']
    return out


def classification_problems(classes=None, structs=None, funcs=None):
    """Every way in which the table and the header disagree: an unclassified pointer, an entry for a pointer the header does not
    have, a stream entry without a row-length source, a guarded entry without a citation or whose cited text is not in its file."""
    classes = CLASSES if classes is None else classes
    if structs is None:
        structs, funcs = A.parse_header()
    bad = []
    want = float_read_pointers(structs, funcs)
    for key in want:
        if key not in classes:
            bad.append(f'{key[0]}: {key[1]} has no slack class')
    for key in classes:
        if key not in want:
            bad.append(f'{key[0]}: {key[1]} is classified but is no const float* of tamgcn.h')
    texts = {}
    for (owner, name), e in classes.items():
        where = f'{owner}: {name}'
        if e.cls not in (STREAM, GUARDED, FLAT):
            bad.append(f'{where}: unknown class {e.cls!r}')
        if e.cls == STREAM:
            decls = structs.get(owner) or funcs.get(owner) or []
            names = {d.name: d for d in decls}
            if e.v == 'desc':
                ok = owner in structs and 'V' in names
            elif e.v and e.v.startswith('arg:'):
                d = names.get(e.v[4:])
                ok = owner in funcs and d is not None and (d.name == 'V' or (d.kind == 'desc' and any(f.name == 'V' for f in structs[d.base])))
            else:
                ok = False
            if not ok:
                bad.append(f'{where}: stream without a row-length source ({e.v!r})')
        if e.cls == GUARDED and not e.cites:
            bad.append(f'{where}: guarded without a citation')
        if e.cls == FLAT and not e.why:
            bad.append(f'{where}: flat without a reason')
        for fname, text in e.cites:
            if fname not in texts:
                path = os.path.join(CSRC, fname)
                texts[fname] = open(path).read() if os.path.exists(path) else None
            if texts[fname] is None:
                bad.append(f'{where}: cites csrc/{fname}, which does not exist')
            elif text not in texts[fname]:
                bad.append(f'{where}: {text!r} is not in csrc/{fname}')
    return bad


def stream_owners(structs=None, funcs=None, classes=None):
    """{entry point: [role]}: the launching entry points (those with a stream parameter) that own a `stream` pointer, directly or
    through a descriptor they take."""
    classes = CLASSES if classes is None else classes
    if structs is None:
        structs, funcs = A.parse_header()
    out = {}
    for fn, params in funcs.items():
        if not any(d.kind == 'stream' for d in params):
            continue
        roles = [name for (owner, name), e in classes.items() if owner == fn and e.cls == STREAM]
        for d in params:
            if d.kind == 'desc' and d.base != 'tamgcn_src':
                roles += [f'{d.name}.{name}' for (owner, name), e in classes.items() if owner == d.base and e.cls == STREAM]
        if roles:
            out[fn] = roles
    return out


# =====================================================================================================================
# the auditor
# =====================================================================================================================
class SlackError(AssertionError):
    def __init__(self, entry, role, shape, behind):
        self.entry, self.role, self.shape, self.behind = entry, role, shape, behind
        AssertionError.__init__(self, f'{entry}: {role} of shape {tuple(shape) if shape is not None else "?"} has {behind} readable '
                                      f'bytes behind its last element in its storage, the 16-byte kernels need {SLACK_BYTES}')


class SlackAuditor(A.LibraryTap):
    """with SlackAuditor() as aud: ...
      aud.launches    [dict(entry, V, ragged, roles {role of a stream pointer: bytes behind}, kernel)] of every library launch
      aud.unresolved  [(entry, role, address)] stream pointers of ragged launches that no tensor seen by the audit contains
      aud.copies      [(shape of the source, 'file:line' of the caller)] of every copy ops.with_slack made
      aud.violations  [(launches made when it was raised, the SlackError)]
    lib: a stand-in for the loaded library (CPU tests).  A tensor is seen when Python takes its data_ptr() -- ops._ptr and the
    eval families' own descriptors do; the extent of the storage is the torch storage's, as ops.with_slack reads it."""

    def __init__(self, lib=None):
        A.LibraryTap.__init__(self, lib)
        self.launches, self.copies, self.violations = [], [], []
        self._seen = {}                                    # data_ptr -> (tensor end, storage end, shape), the last tensor seen there

    # ---- tensors ----------------------------------------------------------------------------------------------------
    def _see(self, t):
        n = t.numel() * t.element_size()
        if not n or not t.is_contiguous():
            return
        st = t.untyped_storage()
        lo = st.data_ptr() + t.storage_offset() * t.element_size()
        self._seen[lo] = (lo + n, st.data_ptr() + st.nbytes(), tuple(t.shape))
        self._register_tensor(t)

    def _register_tensor(self, t):
        n = t.numel() * t.element_size()
        if n:
            st = t.untyped_storage()
            lo = st.data_ptr() + t.storage_offset() * t.element_size()
            self._tensors.add(lo, lo + n)

    def _holder(self, p):
        """(tensor end, storage end, shape) of the tensor that contains address p, or None."""
        hit = self._seen.get(p)
        if hit is not None:
            return hit
        rng = self._tensors.find(p)                        # an offset into a tensor: part.data_ptr() + off
        if rng is not None and rng[0] in self._seen and self._seen[rng[0]][0] == rng[1]:
            return self._seen[rng[0]]
        best = None
        for lo, (hi, send, shape) in self._seen.items():   # ranges of _tensors are disjoint: a later slice may have cut this one
            if lo <= p < hi and (best is None or hi - lo < best[0]):
                best = (hi - lo, (hi, send, shape))
        return best[1] if best else None

    # ---- launches ---------------------------------------------------------------------------------------------------
    def _key_and_v(self, name, role, container, get, field, arg):
        """(table key, row length V) of one pointer of a call."""
        if container.startswith('src:'):
            owner = container[4:]
            key = (owner, f'{field[0]}.{field[1]}')
            getter = get[0]
        elif container == 'tamgcn_src':                    # a tamgcn_src passed as a parameter: role is '<parameter>.<field>'
            key, getter = (name, role), None
        elif container == name:
            key, getter = (name, field), None
        else:
            key, getter = (container, field), get
        e = CLASSES.get(key)
        if e is None or e.cls != STREAM:
            return key, e, None
        if e.v == 'desc':
            return key, e, int(getter('V'))
        a = arg(e.v[4:])
        if isinstance(a, int):
            return key, e, a
        obj = a._obj if hasattr(a, '_obj') else a.contents
        return key, e, int(obj.V)

    def _call(self, name, fn, args):
        params = self._funcs.get(name)
        if params is None or not any(d.kind == 'stream' for d in params):
            return fn(*args)
        _, raw, arg = self._pointers(name, params, args)
        roles, ragged, vs = {}, False, set()
        for p, mode, role, container, get, field in raw:
            if mode != 'r':
                continue
            key, e, V = self._key_and_v(name, role, container, get, field, arg)
            if e is None or e.cls != STREAM:
                continue
            vs.add(V)
            if V % 4 == 0:
                continue
            ragged = True
            hit = self._holder(p)
            if hit is None:
                self.unresolved.append((name, role, p))
                roles[role] = None
                continue
            tend, send, shape = hit
            behind = send - tend
            roles[role] = behind
            if behind < SLACK_BYTES:
                err = SlackError(name, role, shape, behind)
                self.violations.append((len(self.launches), err))
                raise err
        rc = fn(*args)
        kernel = None
        if rc == 0 and self._lib_given is None:
            k = self._real.tamgcn_last_kernel()
            kernel = k.decode(errors='replace') if isinstance(k, bytes) else k
        self.launches.append(dict(entry=name, V=sorted(vs), ragged=ragged, roles=roles, kernel=kernel, rc=rc))
        return rc

    # ---- installation -----------------------------------------------------------------------------------------------
    def __enter__(self):
        import torch
        from tam_gcn_amd import ops
        aud = self
        self._install_library()
        real_data_ptr = torch.Tensor.data_ptr

        def data_ptr(t):
            p = real_data_ptr(t)
            if p:
                aud._see(t)
            return p
        self._patch(torch.Tensor, 'data_ptr', data_ptr)
        real_with_slack = ops.with_slack

        def with_slack(t):
            out = real_with_slack(t)
            if out is not t:
                f = sys._getframe(1)
                while f is not None and f.f_code.co_filename == ops.__file__ and f.f_code.co_name in ('_dy_with_slack',):
                    f = f.f_back
                site = f'{os.path.basename(f.f_code.co_filename)}:{f.f_lineno}' if f is not None else '?'
                aud.copies.append((tuple(t.shape), site))
            return out
        self._patch(ops, 'with_slack', with_slack)
        return self

    def __exit__(self, *exc):
        self._restore()
        return False

    # ---- queries ----------------------------------------------------------------------------------------------------
    @property
    def lib(self):
        """The wrapped library (what tam_gcn_amd._lib.load() returns while the audit is active)."""
        return self._lib_mod._lib

    def ragged_entries(self):
        return {e['entry'] for e in self.launches if e['ragged'] and e['rc'] == 0}

    def kernels(self):
        return [(e['entry'], e['kernel']) for e in self.launches]


def assert_hostile_size(n):
    """A hostile tensor of n floats: its byte size modulo the caching allocator's 512-byte granule lies in 4 .. 496, so the
    allocator's block has at least 16 physical bytes behind the tensor (12, the farthest a 16-byte piece with one valid float
    reaches, behind the same tensor one float into a storage of n + 1 floats) while the torch storage ends where the tensor ends: a kernel classified wrongly cannot reach unmapped memory."""
    r = (4 * n) % 512
    assert 4 <= r <= 496, f'{n} floats: {4 * n} bytes = {r} mod 512; choose a shape with 4 <= (4 n) % 512 <= 496'
    return n
