"""Test-side driver of the C ABI (include/nr_hip.h): torch tensors in, numpy arrays out.  Used by the
`-m gpu` parity tests so that they exercise exactly the entry points a reference-side binding would."""
import numpy as np
import torch

from neural_renderer_amd import _lib


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def forward(faces, textures=None, S=64, near=0.1, far=100.0, eps=1e-4, background=(0, 0, 0), flags=0,
            return_rgb=False, return_alpha=True, return_depth=False, want_face_inv=False, want_sampling=False,
            faces_z_ref=None, want_visible=True):
    """Runs nr_forward_face_index_map (+ nr_forward_texture_sampling). Returns dict of device tensors."""
    lib = _lib.load()
    f = dev(faces, torch.float32)
    B, F = f.shape[:2]
    out = {'faces': f, 'faces_z_ref': dev(faces_z_ref, torch.float32) if faces_z_ref is not None else None}
    out['visible_faces'] = torch.full((B, F), 77, dtype=torch.uint8, device='cuda') if want_visible else None
    out['face_index_map'] = torch.full((B, S, S), 12345, dtype=torch.int32, device='cuda')
    out['weight_map'] = torch.full((B, S, S, 3), float('nan'), device='cuda')
    out['depth_map'] = torch.full((B, S, S), float('nan'), device='cuda')
    out['face_inv_map'] = torch.full((B, S, S, 3, 3), float('nan'), device='cuda') if want_face_inv else None
    wsb = lib.nr_forward_workspace_bytes(B, F, S)
    assert wsb > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device='cuda')
    _lib.check(lib.nr_forward_face_index_map(
        f.data_ptr(), out['face_index_map'].data_ptr(), out['weight_map'].data_ptr(), out['depth_map'].data_ptr(),
        _lib.ptr(out['face_inv_map']), _lib.ptr(out['visible_faces']), B, F, S, near, far, ws.data_ptr(), wsb,
        _stream()), 'fwd fi')
    out['workspace'] = ws
    ts = 0
    if return_rgb or return_alpha:
        t = bg = None
        per_batch = 0
        if return_rgb:
            t = dev(textures, torch.float32)
            ts = t.shape[2]
            bg = dev(np.asarray(background, np.float32))
            per_batch = int(bg.dim() == 2)
            out['rgb_map'] = torch.full((B, S, S, 3), float('nan'), device='cuda')
            if want_sampling:
                out['sampling_index_map'] = torch.full((B, S, S, 8), -7, dtype=torch.int32, device='cuda')
                out['sampling_weight_map'] = torch.full((B, S, S, 8), float('nan'), device='cuda')
        if return_alpha:
            out['alpha_map'] = torch.full((B, S, S), float('nan'), device='cuda')
        out['textures'] = t
        _lib.check(lib.nr_forward_texture_sampling(
            f.data_ptr(), _lib.ptr(out['faces_z_ref']), _lib.ptr(t), out['face_index_map'].data_ptr(), out['weight_map'].data_ptr(),
            out['depth_map'].data_ptr(), _lib.ptr(out.get('rgb_map')), _lib.ptr(out.get('sampling_index_map')),
            _lib.ptr(out.get('sampling_weight_map')), _lib.ptr(bg), per_batch, _lib.ptr(out.get('alpha_map')),
            B, F, S, ts, eps, flags, _stream()), 'fwd shade')
    out.update(B=B, F=F, S=S, ts=ts, eps=eps, flags=flags)
    return out


def backward(fw, g_rgb=None, g_alpha=None, g_depth=None, use_sampling_maps=False, use_face_inv_map=False, k6_flags=0,
             use_visible=True):
    """Runs K6 / K7 / K8 through the ABI on the residuals of `forward`. Returns (grad_faces, grad_textures)."""
    lib = _lib.load()
    B, F, S, ts = fw['B'], fw['F'], fw['S'], fw['ts']
    grad_faces = torch.full((B, F, 3, 3), float('nan'), device='cuda')
    grad_textures = None
    gr = dev(g_rgb, torch.float32) if g_rgb is not None else None
    ga = dev(g_alpha, torch.float32) if g_alpha is not None else None
    gd = dev(g_depth, torch.float32) if g_depth is not None else None
    if gr is not None or ga is not None:
        wsb = lib.nr_backward_workspace_bytes(B, F, S, int(gr is not None), int(ga is not None))
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device='cuda')
        _lib.check(lib.nr_backward_pixel_map(
            fw['faces'].data_ptr(), fw['face_index_map'].data_ptr(),
            _lib.ptr(fw.get('rgb_map')) if gr is not None else None,
            _lib.ptr(fw.get('alpha_map')) if ga is not None else None, _lib.ptr(gr), _lib.ptr(ga),
            grad_faces.data_ptr(), B, F, S, fw['eps'], int(gr is not None), int(ga is not None), k6_flags,
            _lib.ptr(fw.get('visible_faces')) if use_visible else None, ws.data_ptr(), wsb, _stream()), 'bwd pixel_map')
    else:
        grad_faces.zero_()
    if gr is not None:
        grad_textures = torch.full((B, F, ts, ts, ts, 3), float('nan'), device='cuda')  # K7 stores every element
        sw = fw.get('sampling_weight_map') if use_sampling_maps else None
        si = fw.get('sampling_index_map') if use_sampling_maps else None
        _lib.check(lib.nr_backward_textures(
            fw['face_index_map'].data_ptr(), _lib.ptr(sw), _lib.ptr(si), fw['faces'].data_ptr(),
            _lib.ptr(fw.get('faces_z_ref')), fw['weight_map'].data_ptr(), fw['depth_map'].data_ptr(), gr.data_ptr(),
            grad_textures.data_ptr(),
            B, F, S, ts, fw['eps'], fw['flags'], _stream()), 'bwd textures')
    if gd is not None:
        fim = fw.get('face_inv_map') if use_face_inv_map else None
        _lib.check(lib.nr_backward_depth_map(
            fw['faces'].data_ptr(), fw['depth_map'].data_ptr(), fw['face_index_map'].data_ptr(), _lib.ptr(fim),
            fw['weight_map'].data_ptr(), gd.data_ptr(), grad_faces.data_ptr(), B, F, S, _stream()), 'bwd depth')
    torch.cuda.synchronize()
    return grad_faces, grad_textures


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def backward_fused(fw, g_rgb=None, g_alpha=None, g_depth=None, k6_flags=0, use_visible=True, tex_offset=0, workspace_bytes=None,
                   face_light=None):
    """nr_backward_rasterize (K6 -> K7 -> K8 behind one call) on the residuals of `forward`.
    tex_offset: grad_textures starts that many floats off a 16-byte boundary (1: 4 bytes off the grid).
    workspace_bytes: the size of the workspace handed over (None: what nr_backward_workspace_bytes asks for).
    face_light: per-face light colours (nr_backward_rasterize_lit) -- dict(light=[B, F, 3], textures=the original cubes
    [B, Nf, ts, ts, ts, 3], grad_light=bool): grad_textures is then the original cubes' gradient and a third value, grad_light
    [B, F, 3] or None, is returned."""
    lib = _lib.load()
    B, F, S, ts = fw['B'], fw['F'], fw['S'], fw['ts']
    gr = dev(g_rgb, torch.float32) if g_rgb is not None else None
    ga = dev(g_alpha, torch.float32) if g_alpha is not None else None
    gd = dev(g_depth, torch.float32) if g_depth is not None else None
    grad_faces = torch.full((B, F, 3, 3), float('nan'), device='cuda')
    grad_textures = grad_light = lit = None
    keep = []
    if gr is not None:
        shape = (B, F, ts, ts, ts, 3)
        if face_light is not None:
            light, cubes = dev(face_light['light'], torch.float32), dev(face_light['textures'], torch.float32)
            keep += [light, cubes]
            shape = tuple(cubes.shape)
            if face_light.get('grad_light'):
                grad_light = torch.full((B, F, 3), float('nan'), device='cuda')
            lit = _lib.FaceLight(light.data_ptr(), shape[1], cubes.data_ptr(), _lib.ptr(grad_light))
        n = int(np.prod(shape))
        flat = torch.full((n + 4,), float('nan'), device='cuda')
        grad_textures = flat[tex_offset:tex_offset + n].view(shape)
        assert grad_textures.data_ptr() % 16 == 4 * tex_offset % 16
    wsb = lib.nr_backward_workspace_bytes(B, F, S, int(gr is not None), int(ga is not None)) if workspace_bytes is None \
        else workspace_bytes
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device='cuda')
    args = (fw['faces'].data_ptr(), _lib.ptr(fw.get('faces_z_ref')), fw['face_index_map'].data_ptr(),
            _lib.ptr(fw.get('weight_map')), _lib.ptr(fw.get('depth_map')), _lib.ptr(fw.get('rgb_map')),
            _lib.ptr(fw.get('alpha_map')), _lib.ptr(gr), _lib.ptr(ga), _lib.ptr(gd), grad_faces.data_ptr(),
            _lib.ptr(grad_textures), B, F, S, ts, fw['eps'], fw['flags'] | k6_flags,
            _lib.ptr(fw.get('visible_faces')) if use_visible else None, ws.data_ptr(), wsb, _stream())
    if face_light is None:
        _lib.check(lib.nr_backward_rasterize(*args), 'bwd fused')
    else:
        _lib.check(lib.nr_backward_rasterize_lit(lit, *args), 'bwd fused lit')
    torch.cuda.synchronize()
    if grad_textures is not None:  # the guard words around grad_textures: a 16-byte fill must not round its ends outwards
        n = grad_textures.numel()
        assert bool(torch.isnan(flat[:tex_offset]).all()) and bool(torch.isnan(flat[tex_offset + n:]).all()), 'a store outside grad_textures'
    if face_light is not None:
        return grad_faces, grad_textures, grad_light
    return grad_faces, grad_textures


def forward_fused(faces, textures=None, S=64, near=0.1, far=100.0, eps=1e-4, background=(0, 0, 0), flags=0,
                  return_rgb=False, return_alpha=True, return_depth=False, faces_z_ref=None, workspace=None):
    """nr_forward_rasterize (visibility + shading behind one call).  workspace: a kept scratch tensor (NR_FLAG_ZBUF_EPOCH calls)."""
    lib = _lib.load()
    f = dev(faces, torch.float32)
    B, F = f.shape[:2]
    out = {'faces': f, 'faces_z_ref': dev(faces_z_ref, torch.float32) if faces_z_ref is not None else None,
           'visible_faces': torch.full((B, F), 77, dtype=torch.uint8, device='cuda'),
           'face_index_map': torch.full((B, S, S), 12345, dtype=torch.int32, device='cuda'),
           'weight_map': torch.full((B, S, S, 3), float('nan'), device='cuda'),
           'depth_map': torch.full((B, S, S), float('nan'), device='cuda')}
    t = bg = None
    ts, per_batch = 0, 0
    if return_rgb:
        t = dev(textures, torch.float32)
        ts = t.shape[2]
        bg = dev(np.asarray(background, np.float32))
        per_batch = int(bg.dim() == 2)
        out['rgb_map'] = torch.full((B, S, S, 3), float('nan'), device='cuda')
    if return_alpha:
        out['alpha_map'] = torch.full((B, S, S), float('nan'), device='cuda')
    wsb = lib.nr_forward_workspace_bytes(B, F, S)
    ws = workspace if workspace is not None else torch.empty(wsb, dtype=torch.uint8, device='cuda')
    _lib.check(lib.nr_forward_rasterize(
        f.data_ptr(), _lib.ptr(out['faces_z_ref']), _lib.ptr(t), out['face_index_map'].data_ptr(),
        out['weight_map'].data_ptr(), out['depth_map'].data_ptr(), _lib.ptr(out.get('rgb_map')),
        _lib.ptr(out.get('alpha_map')), out['visible_faces'].data_ptr(), _lib.ptr(bg), per_batch, B, F, S, ts, near, far,
        eps, flags, ws.data_ptr(), wsb, _stream()), 'fwd fused')
    torch.cuda.synchronize()
    out.update(B=B, F=F, S=S, ts=ts, eps=eps, flags=flags, textures=t)
    return out
