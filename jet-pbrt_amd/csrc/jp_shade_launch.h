// jet-pbrt_amd/csrc/jp_shade_launch.h -- the launch of k_shade and its families: shade_launch, the one function of the host code that names the k_shade* instantiations,
// and launch_normal, the normal pre-pass of a smooth scene.  jp_render.h declares both (shade_choice, which picks the instance, is defined there); the kernels live with
// their features (jp_kernels.hip, jp_pick.h, jp_env.h, jp_mis.h, jp_normal_map.h, jp_normals.h), so this file is included by jp_kernels.hip after the last of them.
#pragma once
namespace
{
// k_normal; a mapped scene's k_normal_map, or its twin where a map has an active sampling record (jp_tex_sampling.h); with profiling, timed inside the CLS_SHADE pair
static void launch_normal(JpContext* c, const ScenePlan& p, int grid, int cur, const NormView& nv)
{
	Stamper t(c, p.mapped ? CLS_NMAP : CLS_NORMAL);
	if (p.mapped && p.sm.map) hipLaunchKernelGGL(k_normal_map_s, dim3(grid), dim3(JP_BLOCK), 0, c->stream, p.sv, c->q, cur, nv, p.mp, p.sm);
	else if (p.mapped) hipLaunchKernelGGL(k_normal_map, dim3(grid), dim3(JP_BLOCK), 0, c->stream, p.sv, c->q, cur, nv, p.mp);   // normal maps: one kernel leaves Ns or Ns'
	else hipLaunchKernelGGL(k_normal, dim3(grid), dim3(JP_BLOCK), 0, c->stream, p.sv, c->q, cur, nv);
}

// a kernel of the family bound to the views its own signature names, in its own order: a view it does not take cannot reach it
template <class... V>
ShadeLaunch bind_shade(void (*k)(SceneView, Queues, RenderConst, int, DevCounters*, V...), const ShadeViews& all)
{
	return [=](hipStream_t stream, int grid, size_t lds, const SceneView& sv, const Queues& q, const RenderConst& rc, int cur, DevCounters* cnt)
	{ hipLaunchKernelGGL(k, dim3(grid), dim3(JP_BLOCK), lds, stream, sv, q, rc, cur, cnt, std::get<V>(all)...); };
}

// (row, sort) -> f(kTab, kPrims, kStage, kSort) as compile-time booleans: the five rows and two sort variants every family exists in
template <class F> ShadeLaunch by_shade_row(int row, bool sort, F f)
{
	const std::true_type T; const std::false_type N;
	const auto by_sort = [&](auto tab, auto prims, auto stage) { return sort ? f(tab, prims, stage, T) : f(tab, prims, stage, N); };
	switch (row)
	{
	case ROW_TTT: return by_sort(T, T, T);
	case ROW_TTF: return by_sort(T, T, N);
	case ROW_TFT: return by_sort(T, N, T);
	case ROW_TFF: return by_sort(T, N, N);
	default: return by_sort(N, N, N);
	}
}

ShadeLaunch shade_launch(const ShadeChoice& c, const ShadeViews& v)
{
	if (c.family == SHADE_LEAN_ONE) return bind_shade(k_shade_lean_one, v);
	if (c.family == SHADE_LEAN) return c.sort ? bind_shade(k_shade<true, true, true, true, FeatLean>, v) : bind_shade(k_shade<true, true, true, false, FeatLean>, v);
	if (c.smooth)
	{   // the smooth twins: sort alone (their row is ROW_FFF)
		const auto twin = [&](auto sort)
		{
			constexpr bool S = decltype(sort)::value;
			switch (c.family)
			{
			case SHADE_MIS_ENV: return c.tex ? bind_shade(k_shade_smooth_mis_env_tex<S>, v) : bind_shade(k_shade_smooth_mis_env<S>, v);
			case SHADE_MIS: return c.tex ? bind_shade(k_shade_smooth_mis_tex<S>, v) : bind_shade(k_shade_smooth_mis<S>, v);
			case SHADE_ENV: return c.tex ? bind_shade(k_shade_smooth_env_tex<S>, v) : bind_shade(k_shade_smooth_env<S>, v);
			case SHADE_PICK: return c.tex ? bind_shade(k_shade_smooth_pick_tex<S>, v) : bind_shade(k_shade_smooth_pick<S>, v);
			default: return c.tex ? bind_shade(k_shade_smooth_tex<S>, v) : bind_shade(k_shade_smooth<S>, v);
			}
		};
		return c.sort ? twin(std::true_type()) : twin(std::false_type());
	}
	return by_shade_row(c.row, c.sort, [&](auto tab, auto prims, auto stage, auto sort)
	{
		constexpr bool A = decltype(tab)::value, P = decltype(prims)::value, G = decltype(stage)::value, S = decltype(sort)::value;
		switch (c.family)
		{
		case SHADE_MIS_ENV: return c.tex ? bind_shade(k_shade_mis_env_tex<A, P, G, S>, v) : bind_shade(k_shade_mis_env<A, P, G, S>, v);
		case SHADE_MIS: return c.tex ? bind_shade(k_shade_mis_tex<A, P, G, S>, v) : bind_shade(k_shade_mis<A, P, G, S>, v);
		case SHADE_ENV: return c.tex ? bind_shade(k_shade_env_tex<A, P, G, S>, v) : bind_shade(k_shade_env<A, P, G, S>, v);
		case SHADE_PICK: return c.tex ? bind_shade(k_shade_pick_tex<A, P, G, S>, v) : bind_shade(k_shade_pick<A, P, G, S>, v);
		default: return c.tex ? bind_shade(k_shade_tex<A, P, G, S>, v) : bind_shade(k_shade<A, P, G, S>, v);
		}
	});
}
}
