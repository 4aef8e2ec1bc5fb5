/*
 * A part of rtx_trace.hip's translation unit, included there once and not self-contained: it calls the device
 * intersectors and samplers k_trace and k_shadow run (rtx_math.h, rtx_wave.h) on caller-given records.
 */
__global__ void k_kat(int kind, uint32_t n, const float *__restrict__ in, float *__restrict__ out, int u32mode)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	const int wi = rtx_kat_in_width[kind], wo = rtx_kat_out_width[kind];
	const float *x = in + (size_t)i * wi;
	float *y = out + (size_t)i * wo;
	for (int k = 0; k < wo; k++)
		y[k] = 0.f;
	switch (kind) {
	case RTX_KAT_MOLLER: {
		float t = 0.f;
		bool h = hit_triangle(ld3(x + 6), ld3(x + 9), ld3(x + 12), ld3(x), ld3(x + 3), x[15], t);
		y[0] = h;
		y[1] = h ? t : 0.f;
	} break;
	case RTX_KAT_SPHERE: {
		float t = 0.f;
		f3 o = ld3(x), d = ld3(x + 3), c = ld3(x + 6);
		bool h = hit_sphere(c, x[9], o, d, x[10], t);
		y[0] = h;
		if (h) {
			y[1] = t;
			f3 n = mul3s(sub3(add3(mul3s(d, t), o), c), 1.f / x[9]);
			y[2] = n.x;
			y[3] = n.y;
			y[4] = n.z;
		}
	} break;
	case RTX_KAT_PLANE: {
		float t = 0.f;
		f3 o = ld3(x), d = ld3(x + 3), nn = ld3(x + 6);
		bool h = hit_plane(nn, x[9], o, d, x[10], t);
		y[0] = h;
		if (h) {
			y[1] = t;
			f3 n = signbit(dot3(nn, d)) ? nn : mul3s(nn, -1.f);
			y[2] = n.x;
			y[3] = n.y;
			y[4] = n.z;
		}
	} break;
	case RTX_KAT_SLAB: {
		float tmin = 0.f, tmax = 0.f;
		bool h = slab_ref(ld3(x + 6), ld3(x + 9), x[12], ld3(x), ld3(x + 3), tmin, tmax);
		y[0] = h;
		y[1] = h ? tmin : 0.f;
		y[2] = h ? tmax : 0.f;
	} break;
	case RTX_KAT_NOISE:
		y[0] = simplex3(x[0], x[1], x[2]);
		break;
	case RTX_KAT_TEXTURE: {
		DMaterial m;
		m.tex = (int)x[0];
		m.periodic = (int)x[1];
		for (int k = 0; k < 3; k++) {
			m.color[0][k] = x[2 + k];
			m.color[1][k] = x[5 + k];
		}
		m.scale = x[8];
		m.mortar = x[9];
		m.nfs = x[10];
		m.ns = x[11];
		m.fs = x[12];
		f3 c = texture_color(m, ld3(x + 13), u32mode);
		y[0] = c.x;
		y[1] = c.y;
		y[2] = c.z;
	} break;
	case RTX_KAT_SPH_LIGHT:
	case RTX_KAT_TRI_LIGHT: {
		DEmitter e;
		f3 p = mk3(0.f, 0.f, 0.f);
		float u1, u2;
		if (kind == RTX_KAT_SPH_LIGHT) {
			e.type = RTX_SPHERE;
			for (int k = 0; k < 3; k++)
				e.p0[k] = x[k];
			e.radius = x[3];
			p = ld3(x + 4);
			u1 = x[7];
			u2 = x[8];
		} else {
			e.type = RTX_TRIANGLE;
			for (int k = 0; k < 3; k++) {
				e.p0[k] = x[k];
				e.p1[k] = x[3 + k];
				e.p2[k] = x[6 + k];
			}
			u1 = x[9];
			u2 = x[10];
		}
		f3 l = light_point(e, p, u1, u2);
		y[0] = l.x;
		y[1] = l.y;
		y[2] = l.z;
	} break;
	case RTX_KAT_MORTON: {
		/* accel.c:72-88 (used by the reference's BVH build; kept for parity of the KAT suite) */
		uint32_t c = 0;
		for (int a = 0; a < 3; a++) {
			uint32_t v = (uint32_t)(1023.f * x[a]);
			v = (v * 0x00010001u) & 0xFF0000FFu;
			v = (v * 0x00000101u) & 0x0F00F00Fu;
			v = (v * 0x00000011u) & 0xC30C30C3u;
			v = (v * 0x00000005u) & 0x49249249u;
			c += v * (a == 0 ? 4u : a == 1 ? 2u : 1u);
		}
		y[0] = __uint_as_float(c);
	} break;
	case RTX_KAT_U32:
		y[0] = __uint_as_float(to_u32(x[0], RTX_U32_SAT));
		y[1] = __uint_as_float(to_u32(x[0], RTX_U32_WRAP));
		break;
	case RTX_KAT_GI_DIR: {
		f3 dd = gi_direction(ld3(x), x[3], x[4], x[5]);
		y[0] = dd.x;
		y[1] = dd.y;
		y[2] = dd.z;
	} break;
	case RTX_KAT_REFRACT: {
		f3 dd = ld3(x), nn = ld3(x + 3);
		float b = dot3(nn, dd);
		f3 r = refract_dir(dd, nn, b, signbit(b), x[6]);
		y[0] = r.x;
		y[1] = r.y;
		y[2] = r.z;
	} break;
	}
}
