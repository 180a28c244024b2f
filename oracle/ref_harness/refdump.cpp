// refdump — headless harness around the UNMODIFIED reference sources (clayne/CPU-Raytracer).
//
// TEST INFRASTRUCTURE ONLY.  Built by oracle/ref_harness/Makefile from the sources where they lie
// under /root/reference (nothing is copied into this repo); the binary lands in oracle/_ref/.
// It exists to (a) pin oracle/rt_oracle.c against the real reference and (b) dump scenes in this
// repo's own scene format (python: cpu-raytracer_amd/pyrtx/scene_io.py) together with golden
// framebuffers.  Nothing in the product path may link or run it.
//
// What it does: reads a small scene script, drives the reference's own public objects
//   Texture::init / MaterialBuffer::init / Scene / Camera::resize / Scene::update /
//   Raytracer::render_tile / Raytracer::bounce            (Main.cpp:25-57, Raytracer.h:11-18)
// at SIMD_LANE_SIZE == 1 and writes:
//   scene.rtxs   scene after Scene::update, in this repo's chunk format
//   rgb.f32      W*H*3 fp32 linear colours = return value of Raytracer::bounce per pixel
//   packed.u32   W*H packed pixels written by Raytracer::render_tile through Window::plot
//   stats.json   PerformanceStats of both passes, timings
//
// The only reference behaviour restated here is the 10-line primary-ray set-up needed to call
// bounce() directly (Raytracer.cpp:45-59); it is cross-checked against render_tile's packed output
// for every pixel on every run (see check_packed below).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>
#include <chrono>
#include <thread>
#include <atomic>
#include <sstream>
#include <fstream>
#include <map>
#include <unordered_map>
#include <algorithm>
#include <filesystem>

// The harness must read a few private fields (Sphere radius, Plane axes, Texture texels, Sky
// texels) and call the private Raytracer::bounce.  Access control is lifted for THIS translation
// unit only; the reference's own translation units are compiled untouched.
#define private public
#include "Raytracer.h"
#undef private

#include "../../include/rtx.h"
#ifdef REFBIND
#include "WorkerThread.h"      // the four WorkerThreads entry points; implemented by GpuBackend.cpp in this build (refbind_* binaries)
#endif

// ---- headless Window (Window.cpp is SDL/GL and is not compiled) -------------------------------
Window::Window(int width, int height, const char * title) :
	width(width), height(height),
	tile_count_x((width  + tile_width  - 1) / tile_width),
	tile_count_y((height + tile_height - 1) / tile_height)
{
	frame_buffer = new unsigned[width * height];
	memset(frame_buffer, 0, sizeof(unsigned) * width * height);
}
Window::~Window() { delete [] frame_buffer; }

// Scene::update polls the keyboard (Scene.cpp:165).  Headless: no key is down unless the script holds some (`keys ...`).
static Uint8 no_keys[SDL_NUM_SCANCODES];
extern "C" const Uint8 * SDL_GetKeyboardState(int * numkeys) { if (numkeys) *numkeys = SDL_NUM_SCANCODES; return no_keys; }   // script command `keys` presses some

// ---- chunk writer ------------------------------------------------------------------------------
struct ChunkWriter {
	FILE * f;
	explicit ChunkWriter(const std::string & path) {
		f = fopen(path.c_str(), "wb");
		if (!f) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(2); }
		fwrite("RTXSCN01", 1, 8, f);
	}
	~ChunkWriter() { fclose(f); }
	void chunk(const char tag[5], uint32_t n, const void * data, uint64_t nbytes) {
		fwrite(tag, 1, 4, f);
		fwrite(&n, 4, 1, f);
		fwrite(&nbytes, 8, 1, f);
		if (nbytes) fwrite(data, 1, nbytes, f);
		static const char zeros[8] = {0};
		uint64_t pad = (8 - (nbytes & 7)) & 7;
		if (pad) fwrite(zeros, 1, pad, f);
	}
};

static void v3(float * dst, const Vector3 & v) { dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; }
static void v3(float * dst, const SIMD_Vector3 & v) { dst[0] = v.x[0]; dst[1] = v.y[0]; dst[2] = v.z[0]; }

struct MeshSpec { std::string path; Vector3 pos; Quaternion rot; };

struct MatEdit { std::string target; std::string field; std::vector<std::string> args; };

static std::vector<std::string> split(const std::string & s) {
	std::istringstream is(s); std::vector<std::string> out; std::string w;
	while (is >> w) out.push_back(w);
	return out;
}

static Scene * g_scene;

static int resolve_material(const std::string & target) {
	// mesh:<i>:<local>, sphere:<i>, plane:<i>, global:<id>
	std::vector<std::string> parts; { std::string t = target; size_t p; while ((p = t.find(':')) != std::string::npos) { parts.push_back(t.substr(0, p)); t = t.substr(p + 1); } parts.push_back(t); }
	if (parts[0] == "mesh")   return g_scene->top_level_bvh.primitives[atoi(parts[1].c_str())].bvh->material_offset + atoi(parts[2].c_str());
	if (parts[0] == "sphere") return g_scene->spheres[atoi(parts[1].c_str())].material_id;
	if (parts[0] == "plane")  return g_scene->planes [atoi(parts[1].c_str())].material_id;
	if (parts[0] == "global") return atoi(parts[1].c_str());
	fprintf(stderr, "bad material target %s\n", target.c_str()); exit(2);
}

int main(int argc, char ** argv) {
	if (argc < 3) { fprintf(stderr, "usage: refdump <script> <outdir> [--threads N]\n  (cwd must contain ./Data as the reference expects, Util.h:6)\n"); return 2; }
	std::string script = argv[1], outdir = argv[2];
	int mt_threads = 0, mt_frames = 3; bool timing_only = false;           // --threads N [--frames K] [--timing-only]: the reference's worker pool, timed
	int binding_frames = 0; float binding_delta = 1.0f / 60.0f;            // --gpu-binding N [--binding-delta s]: refbind_* builds only, see below
	for (int a = 3; a < argc; a++) {
		if (!strcmp(argv[a], "--gpu-binding") && a + 1 < argc) { binding_frames = atoi(argv[++a]); continue; }
		if (!strcmp(argv[a], "--binding-delta") && a + 1 < argc) { binding_delta = (float)atof(argv[++a]); continue; }
		if (!strcmp(argv[a], "--threads") && a + 1 < argc) mt_threads = atoi(argv[++a]);
		else if (!strcmp(argv[a], "--frames") && a + 1 < argc) mt_frames = atoi(argv[++a]);
		else if (!strcmp(argv[a], "--timing-only")) timing_only = true;
	}
	std::filesystem::create_directories(outdir);

	int W = 256, H = 256, bounces = NUMBER_OF_BOUNCES, frames = 1; float delta = 0.0f;
	int unit_n = 0; unsigned unit_seed = 1;
	std::string rayprobe_path; int rayprobe_n = 0;
	std::string shadeprobe_path; int shadeprobe_n = 0;
	bool keep_base = false, drop_base_meshes = false, have_camera = false, have_ambient = false;
	Vector3 cam_pos; Quaternion cam_rot; Vector3 ambient;
	std::vector<MeshSpec> meshes;
	struct SphereSpec { Vector3 c; float r; }; std::vector<SphereSpec> spheres;
	struct PlaneSpec { Vector3 p; Quaternion q; }; std::vector<PlaneSpec> planes;
	struct PL { Vector3 c, p; }; std::vector<PL> pls;
	struct SL { Vector3 c, p, d; float in, out; }; std::vector<SL> sls;
	struct DL { Vector3 c, d; }; std::vector<DL> dls;
	bool lights_given = false;
	std::vector<MatEdit> edits;
	struct TexProbe { std::string path; int n; unsigned seed; }; std::vector<TexProbe> probes;
	struct TexProbeFile { std::string path, inputs; }; std::vector<TexProbeFile> file_probes;
	int render_reps = 1;

	{
		std::ifstream in(script);
		if (!in) { fprintf(stderr, "cannot read %s\n", script.c_str()); return 2; }
		std::string line;
		while (std::getline(in, line)) {
			size_t h = line.find('#'); if (h != std::string::npos) line = line.substr(0, h);
			std::vector<std::string> w = split(line); if (w.empty()) continue;
			auto F = [&](int i) { return (float)atof(w[i].c_str()); };
			if      (w[0] == "size")    { W = atoi(w[1].c_str()); H = atoi(w[2].c_str()); }
			else if (w[0] == "bounces") { bounces = atoi(w[1].c_str()); }
			else if (w[0] == "frames")  { frames = atoi(w[1].c_str()); delta = F(2); }
			else if (w[0] == "reps")    { render_reps = atoi(w[1].c_str()); }
			else if (w[0] == "keys")    {   // held down during every Scene::update (Camera::update, Camera.cpp:18-48)
				for (size_t k = 1; k < w.size(); k++) {
					int sc = w[k] == "W" ? SDL_SCANCODE_W : w[k] == "A" ? SDL_SCANCODE_A : w[k] == "S" ? SDL_SCANCODE_S : w[k] == "D" ? SDL_SCANCODE_D :
					         w[k] == "LSHIFT" ? SDL_SCANCODE_LSHIFT : w[k] == "SPACE" ? SDL_SCANCODE_SPACE : w[k] == "UP" ? SDL_SCANCODE_UP :
					         w[k] == "DOWN" ? SDL_SCANCODE_DOWN : w[k] == "LEFT" ? SDL_SCANCODE_LEFT : w[k] == "RIGHT" ? SDL_SCANCODE_RIGHT : -1;
					if (sc < 0) { fprintf(stderr, "unknown key %s\n", w[k].c_str()); return 2; }
					no_keys[sc] = 1;
				}
			}
			else if (w[0] == "base")    { keep_base = (w[1] == "keep"); }
			else if (w[0] == "drop_base_meshes") { drop_base_meshes = true; }
			else if (w[0] == "camera")  { have_camera = true; cam_pos = Vector3(F(1), F(2), F(3)); cam_rot = Quaternion(F(4), F(5), F(6), F(7)); }
			else if (w[0] == "camera_axis_angle") { have_camera = true; cam_pos = Vector3(F(1), F(2), F(3)); cam_rot = Quaternion::axis_angle(Vector3(F(4), F(5), F(6)), F(7)); }
			else if (w[0] == "ambient") { have_ambient = true; ambient = Vector3(F(1), F(2), F(3)); }
			else if (w[0] == "mesh")    { MeshSpec m; m.path = w[1]; m.pos = Vector3(F(2), F(3), F(4)); m.rot = w.size() >= 9 ? Quaternion(F(5), F(6), F(7), F(8)) : Quaternion(); meshes.push_back(m); }
			else if (w[0] == "mesh_axis_angle") { MeshSpec m; m.path = w[1]; m.pos = Vector3(F(2), F(3), F(4)); m.rot = Quaternion::axis_angle(Vector3(F(5), F(6), F(7)), F(8)); meshes.push_back(m); }
			else if (w[0] == "sphere")  { spheres.push_back({ Vector3(F(1), F(2), F(3)), F(4) }); }
			else if (w[0] == "plane")   { planes.push_back({ Vector3(F(1), F(2), F(3)), w.size() >= 8 ? Quaternion(F(4), F(5), F(6), F(7)) : Quaternion() }); }
			else if (w[0] == "plane_axis_angle") { planes.push_back({ Vector3(F(1), F(2), F(3)), Quaternion::axis_angle(Vector3(F(4), F(5), F(6)), F(7)) }); }
			else if (w[0] == "point")   { lights_given = true; pls.push_back({ Vector3(F(1), F(2), F(3)), Vector3(F(4), F(5), F(6)) }); }
			else if (w[0] == "spot")    { lights_given = true; sls.push_back({ Vector3(F(1), F(2), F(3)), Vector3(F(4), F(5), F(6)), Vector3(F(7), F(8), F(9)), F(10), F(11) }); }
			else if (w[0] == "dir")     { lights_given = true; dls.push_back({ Vector3(F(1), F(2), F(3)), Vector3(F(4), F(5), F(6)) }); }
			else if (w[0] == "nolights") { lights_given = true; }
			else if (w[0] == "matset")  { MatEdit e; e.target = w[1]; e.field = w[2]; e.args.assign(w.begin() + 3, w.end()); edits.push_back(e); }
			else if (w[0] == "texprobe") { probes.push_back({ w[1], atoi(w[2].c_str()), (unsigned)strtoul(w[3].c_str(), nullptr, 0) }); }
			else if (w[0] == "texprobe_file") { file_probes.push_back({ w[1], w[2] }); }
			else if (w[0] == "unitprobe") { unit_n = atoi(w[1].c_str()); unit_seed = (unsigned)strtoul(w[2].c_str(), nullptr, 0); }
			else if (w[0] == "rayprobe")  { rayprobe_path = w[1]; rayprobe_n = atoi(w[2].c_str()); }
			else if (w[0] == "shadeprobe") { shadeprobe_path = w[1]; shadeprobe_n = atoi(w[2].c_str()); }
			else { fprintf(stderr, "unknown script command '%s'\n", w[0].c_str()); return 2; }
		}
	}

	// ---- Main.cpp:18-40 ---------------------------------------------------------------------------
	Window window(W, H, "refdump");
	Texture::init();
	MaterialBuffer::init();

	Scene scene; g_scene = &scene;
	scene.camera.resize(W, H);

	if (!keep_base) {
		scene.spheres.primitive_count = 0;
		scene.planes.primitive_count  = 0;
	}
	if (!spheres.empty()) {
		int base = keep_base ? scene.spheres.primitive_count : 0;
		Sphere * s = new Sphere[base + spheres.size()];
		for (int i = 0; i < base; i++) s[i] = scene.spheres.primitives[i];
		for (size_t i = 0; i < spheres.size(); i++) { s[base + i].init(spheres[i].r); s[base + i].transform.position = spheres[i].c; }
		scene.spheres.primitives = s; scene.spheres.primitive_count = base + (int)spheres.size();
	}
	if (!planes.empty()) {
		int base = keep_base ? scene.planes.primitive_count : 0;
		Plane * p = new Plane[base + planes.size()];
		for (int i = 0; i < base; i++) p[i] = scene.planes.primitives[i];
		for (size_t i = 0; i < planes.size(); i++) { p[base + i].transform.position = planes[i].p; p[base + i].transform.rotation = planes[i].q; }
		scene.planes.primitives = p; scene.planes.primitive_count = base + (int)planes.size();
	}
	if (!keep_base || !meshes.empty()) {
		int base = (keep_base && !drop_base_meshes) ? scene.top_level_bvh.primitive_count : 0;
		std::vector<Mesh> old(scene.top_level_bvh.primitives, scene.top_level_bvh.primitives + base);
		int n = base + (int)meshes.size();
		if (n == 0) { fprintf(stderr, "script defines no mesh (TopLevelBVH::init asserts count > 0)\n"); return 2; }
		scene.top_level_bvh.init(n);
		for (int i = 0; i < base; i++) scene.top_level_bvh.primitives[i] = old[i];
		for (size_t i = 0; i < meshes.size(); i++) {
			Mesh & m = scene.top_level_bvh.primitives[base + i];
			m.transform.position = meshes[i].pos;
			m.transform.rotation = meshes[i].rot;
			m.init(meshes[i].path.c_str());
		}
	}
	if (lights_given) {
		scene.point_light_count = (int)pls.size();
		scene.point_lights = (PointLight *)malloc(sizeof(PointLight) * (pls.size() + 1));
		for (size_t i = 0; i < pls.size(); i++) new (&scene.point_lights[i]) PointLight(pls[i].c, pls[i].p);
		scene.spot_light_count = (int)sls.size();
		scene.spot_lights = (SpotLight *)malloc(sizeof(SpotLight) * (sls.size() + 1));
		for (size_t i = 0; i < sls.size(); i++) new (&scene.spot_lights[i]) SpotLight(sls[i].c, sls[i].p, Vector3::normalize(sls[i].d), sls[i].in, sls[i].out);
		scene.directional_light_count = (int)dls.size();
		scene.directional_lights = (DirectionalLight *)malloc(sizeof(DirectionalLight) * (dls.size() + 1));
		for (size_t i = 0; i < dls.size(); i++) new (&scene.directional_lights[i]) DirectionalLight(dls[i].c, Vector3::normalize(dls[i].d));
	}
	if (have_camera)  { scene.camera.position = cam_pos; scene.camera.rotation = cam_rot; }
	if (have_ambient) { scene.ambient_lighting = ambient; }

	for (const MatEdit & e : edits) {
		Material & m = MaterialBuffer::materials[resolve_material(e.target)];
		auto F = [&](int i) { return (float)atof(e.args[i].c_str()); };
		if      (e.field == "diffuse")       m.diffuse       = Vector3(F(0), F(1), F(2));
		else if (e.field == "reflection")    m.reflection    = Vector3(F(0), F(1), F(2));
		else if (e.field == "transmittance") m.transmittance = Vector3(F(0), F(1), F(2));
		else if (e.field == "ior")           m.index_of_refraction = F(0);
		else if (e.field == "notexture")     m.texture = nullptr;
		else if (e.field == "texture")       m.texture = Texture::load(e.args[0].c_str());
		else { fprintf(stderr, "bad matset field %s\n", e.field.c_str()); return 2; }
	}

	// ---- Main.cpp:54: Scene::update, `frames` times ---------------------------------------------------
	for (int f = 0; f < frames; f++) scene.update(delta);

	Raytracer raytracer;
	raytracer.scene = &scene;

	// ---- the drop-in binding, executed (refbind_* builds): Main.cpp:51-57's loop with GpuBackend.cpp standing where WorkerThread.cpp
	//      stood, next to the reference's own render_tile loop on the SAME Scene / Window objects.  Per frame: scene.update(delta);
	//      reference tiles -> Window::frame_buffer (kept aside); WorkerThreads::wake_up_worker_threads + wait_on_worker_threads ->
	//      Window::frame_buffer again, through rtx_set_frame / rtx_render_tiles / rtx_read_framebuffer; the two must be equal in every
	//      pixel, and sum_performance_stats() must return the reference's ray counts.
	if (binding_frames > 0) {
#ifdef REFBIND
		if (bounces != NUMBER_OF_BOUNCES) { fprintf(stderr, "--gpu-binding: the script's bounces must equal this build's NUMBER_OF_BOUNCES (%d)\n", NUMBER_OF_BOUNCES); return 2; }
		const int tiles = window.tile_count_x * window.tile_count_y;
		std::vector<unsigned> ref_fb((size_t)W * H);
		std::vector<long> mismatches; std::vector<int> stats_ok; bool identical = true;
		PerformanceStats last_ref = { 0, 0, 0, 0 }, last_gpu = { 0, 0, 0, 0 };
		for (int f = 0; f < binding_frames; f++) {
			scene.update(f == 0 ? 0.0f : binding_delta);                                       // Main.cpp:54
			PerformanceStats sr = { 0, 0, 0, 0 };
			for (int task = tiles - 1; task >= 0; task--) {                                  // WorkerThread.cpp:53-65, one thread
				int x = (task % window.tile_count_x) * window.tile_width, y = (task / window.tile_count_x) * window.tile_height;
				int tw = x + window.tile_width  < window.width  ? window.tile_width  : window.width  - x;
				int th = y + window.tile_height < window.height ? window.tile_height : window.height - y;
				raytracer.render_tile(window, x, y, tw, th, sr);
			}
			memcpy(ref_fb.data(), window.frame_buffer, ref_fb.size() * sizeof(unsigned));
			memset(window.frame_buffer, 0xCD, ref_fb.size() * sizeof(unsigned));
			if (f == 0) WorkerThreads::init(raytracer, window);                                // Main.cpp:46
			WorkerThreads::wake_up_worker_threads(tiles);                                      // Main.cpp:56
			WorkerThreads::wait_on_worker_threads();                                           // Main.cpp:57
			const PerformanceStats sg = WorkerThreads::sum_performance_stats();
			long bad = 0;
			for (size_t p = 0; p < ref_fb.size(); p++) if (ref_fb[p] != window.frame_buffer[p]) bad++;
			const int sok = sr.num_primary_rays == sg.num_primary_rays && sr.num_shadow_rays == sg.num_shadow_rays &&
			                sr.num_reflection_rays == sg.num_reflection_rays && sr.num_refraction_rays == sg.num_refraction_rays;
			mismatches.push_back(bad); stats_ok.push_back(sok); identical = identical && bad == 0 && sok;
			last_ref = sr; last_gpu = sg;
		}
		FILE * jf = fopen((outdir + "/binding.json").c_str(), "w");
		fprintf(jf, "{\"frames\": %d, \"width\": %d, \"height\": %d, \"identical\": %s, \"mismatched_pixels\": [", binding_frames, W, H, identical ? "true" : "false");
		for (size_t i = 0; i < mismatches.size(); i++) fprintf(jf, "%s%ld", i ? ", " : "", mismatches[i]);
		fprintf(jf, "], \"stats_equal\": [");
		for (size_t i = 0; i < stats_ok.size(); i++) fprintf(jf, "%s%s", i ? ", " : "", stats_ok[i] ? "true" : "false");
		fprintf(jf, "],\n \"reference_rays\": [%lld, %lld, %lld, %lld], \"binding_rays\": [%lld, %lld, %lld, %lld], \"instances\": %d, \"simd_lane_size\": %d}\n",
		        (long long)last_ref.num_primary_rays, (long long)last_ref.num_shadow_rays, (long long)last_ref.num_reflection_rays, (long long)last_ref.num_refraction_rays,
		        (long long)last_gpu.num_primary_rays, (long long)last_gpu.num_shadow_rays, (long long)last_gpu.num_reflection_rays, (long long)last_gpu.num_refraction_rays,
		        scene.top_level_bvh.primitive_count, SIMD_LANE_SIZE);
		fclose(jf);
		return identical ? 0 : 4;
#else
		fprintf(stderr, "--gpu-binding needs a refbind_* build (make -C oracle/ref_harness refbind)\n"); return 2;
#endif
	}

	// ---- pass 1: the reference's own tile loop (WorkerThread.cpp:53-65, single thread) ------------
	PerformanceStats stats_tiles = { 0, 0, 0, 0 };
	double best_ms = 1e30;
	static_assert(NUMBER_OF_BOUNCES >= 0, "");
	bool tiles_valid = (bounces == NUMBER_OF_BOUNCES);   // render_tile uses the compile-time constant
	if (tiles_valid) {
		for (int rep = 0; rep < render_reps; rep++) {
			stats_tiles = { 0, 0, 0, 0 };
			auto t0 = std::chrono::high_resolution_clock::now();
			for (int task = window.tile_count_x * window.tile_count_y - 1; task >= 0; task--) {
				int x = (task % window.tile_count_x) * window.tile_width;
				int y = (task / window.tile_count_x) * window.tile_height;
				int tw = x + window.tile_width  < window.width  ? window.tile_width  : window.width  - x;
				int th = y + window.tile_height < window.height ? window.tile_height : window.height - y;
				raytracer.render_tile(window, x, y, tw, th, stats_tiles);
			}
			auto t1 = std::chrono::high_resolution_clock::now();
			best_ms = std::min(best_ms, std::chrono::duration<double, std::milli>(t1 - t0).count());
		}
	}

	// ---- pass 1b: the same loop on N threads pulling tiles from an atomic counter, exactly WorkerThread.cpp:53-65 (Win32 threads
	//      and events replaced by std::thread; each thread owns its PerformanceStats, :110).  Timing only; pixels are identical.
	double mt_best_ms = -1.0; PerformanceStats stats_mt = { 0, 0, 0, 0 };
	if (tiles_valid && mt_threads > 0) {
		mt_best_ms = 1e30;
		for (int rep = 0; rep < mt_frames; rep++) {
			std::atomic<int> remaining(window.tile_count_x * window.tile_count_y);
			std::vector<PerformanceStats> per(mt_threads, PerformanceStats{ 0, 0, 0, 0 });
			std::vector<std::thread> pool;
			auto t0 = std::chrono::high_resolution_clock::now();
			for (int t = 0; t < mt_threads; t++) pool.emplace_back([&, t] {
				for (;;) {
					int task = remaining.fetch_sub(1) - 1;               // _InterlockedDecrement, WorkerThread.cpp:54
					if (task < 0) break;
					int x = (task % window.tile_count_x) * window.tile_width;
					int y = (task / window.tile_count_x) * window.tile_height;
					int tw = x + window.tile_width  < window.width  ? window.tile_width  : window.width  - x;
					int th = y + window.tile_height < window.height ? window.tile_height : window.height - y;
					raytracer.render_tile(window, x, y, tw, th, per[t]);
				}
			});
			for (auto & th : pool) th.join();
			auto t1 = std::chrono::high_resolution_clock::now();
			mt_best_ms = std::min(mt_best_ms, std::chrono::duration<double, std::milli>(t1 - t0).count());
			stats_mt = { 0, 0, 0, 0 };
			for (auto & p : per) { stats_mt.num_primary_rays += p.num_primary_rays; stats_mt.num_shadow_rays += p.num_shadow_rays; stats_mt.num_reflection_rays += p.num_reflection_rays; stats_mt.num_refraction_rays += p.num_refraction_rays; }
		}
	}
	if (timing_only) {
		FILE * f = fopen((outdir + "/timing.json").c_str(), "w");
		fprintf(f, "{\"width\": %d, \"height\": %d, \"threads\": %d, \"frames\": %d, \"render_ms_threads_best\": %.3f, \"render_tile_ms_1thread\": %.3f,\n"
		           " \"primary\": %lld, \"shadow\": %lld, \"reflection\": %lld, \"refraction\": %lld, \"simd_lane_size\": %d}\n",
		        W, H, mt_threads, mt_frames, mt_best_ms, tiles_valid ? best_ms : -1.0,
		        (long long)stats_tiles.num_primary_rays, (long long)stats_tiles.num_shadow_rays, (long long)stats_tiles.num_reflection_rays, (long long)stats_tiles.num_refraction_rays, SIMD_LANE_SIZE);
		fclose(f);
		if (mt_threads > 0 && (stats_mt.num_primary_rays != stats_tiles.num_primary_rays || stats_mt.num_shadow_rays != stats_tiles.num_shadow_rays)) { fprintf(stderr, "thread pool ray counts differ\n"); return 3; }
		return 0;
	}

	// ---- pass 2: bounce() per pixel for fp32 colours ----------------------------------------------
	std::vector<float> rgb((size_t)W * H * 3);
	std::vector<float> dist((size_t)W * H);
	PerformanceStats stats_px = { 0, 0, 0, 0 };
	{
		Ray ray;
		ray.origin = SIMD_Vector3(scene.camera.position);
#if RAY_DIFFERENTIALS_ENABLED
		ray.dO_dx = SIMD_Vector3(0.0f);
		ray.dO_dy = SIMD_Vector3(0.0f);
#endif
		const Camera & c = scene.camera;
		for (int j = 0; j < H; j++) for (int i = 0; i < W; i++) {
			SIMD_float is((float)i), js((float)j);
			SIMD_Vector3 d = SIMD_Vector3::madd(c.rotated_x_axis, is, SIMD_Vector3::madd(c.rotated_y_axis, js, c.rotated_top_left_corner));
			SIMD_float dd = SIMD_Vector3::dot(d, d);
			SIMD_float inv = SIMD_float::inv_sqrt(dd);
			SIMD_float denom = inv / dd;
#if RAY_DIFFERENTIALS_ENABLED
			ray.dD_dx = (dd * c.rotated_x_axis - SIMD_Vector3::dot(d, c.rotated_x_axis) * d) * denom;
			ray.dD_dy = (dd * c.rotated_y_axis - SIMD_Vector3::dot(d, c.rotated_y_axis) * d) * denom;
#endif
			ray.direction = d * inv;
			stats_px.num_primary_rays++;
			SIMD_float distance;
			SIMD_Vector3 colour = raytracer.bounce(ray, bounces, distance, stats_px);
			size_t p = (size_t)j * W + i;
			rgb[3 * p + 0] = colour.x[0]; rgb[3 * p + 1] = colour.y[0]; rgb[3 * p + 2] = colour.z[0];
			dist[p] = distance[0];
		}
	}

	// check_packed: quantising pass 2 exactly as Window::plot does must reproduce pass 1 bit for bit
	long packed_mismatch = -1;
	if (tiles_valid) {
		packed_mismatch = 0;
		Window check(W, H, "check");
		for (int j = 0; j < H; j++) for (int i = 0; i < W; i++) {
			size_t p = (size_t)j * W + i;
			check.plot(i, j, Vector3(rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]));
			if (check.frame_buffer[p] != window.frame_buffer[p]) packed_mismatch++;
		}
		if (stats_tiles.num_primary_rays != stats_px.num_primary_rays || stats_tiles.num_shadow_rays != stats_px.num_shadow_rays ||
		    stats_tiles.num_reflection_rays != stats_px.num_reflection_rays || stats_tiles.num_refraction_rays != stats_px.num_refraction_rays) packed_mismatch += 1000000000L;
	} else {
		// no render_tile pass for this bounce count: quantise pass 2 through Window::plot
		for (int j = 0; j < H; j++) for (int i = 0; i < W; i++) {
			size_t p = (size_t)j * W + i;
			window.plot(i, j, Vector3(rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]));
		}
	}

	// ---- dump scene -----------------------------------------------------------------------------------
	{
		ChunkWriter cw(outdir + "/scene.rtxs");
		rtx_config conf; memset(&conf, 0, sizeof(conf));
		conf.width = W; conf.height = H; conf.bounces = bounces; conf.stack_size = BVH_TRAVERSAL_STACK_SIZE;
		conf.traversal_strategy = BVH_TRAVERSAL_STRATEGY; conf.texture_mode = TEXTURE_SAMPLE_MODE; conf.mip_filter = MIPMAP_FILTER; conf.heatmap = BVH_VISUALIZE_HEATMAP ? 1 : 0;
		conf.max_anisotropy = MAX_ANISOTROPY; conf.device = 0;
		cw.chunk("CONF", 1, &conf, sizeof(conf));

		rtx_camera cam;
		v3(cam.position, scene.camera.position);
		v3(cam.rotated_top_left_corner, scene.camera.rotated_top_left_corner);
		v3(cam.rotated_x_axis, scene.camera.rotated_x_axis);
		v3(cam.rotated_y_axis, scene.camera.rotated_y_axis);
		cw.chunk("CAMR", 1, &cam, sizeof(cam));
		float amb[4] = { scene.ambient_lighting.x, scene.ambient_lighting.y, scene.ambient_lighting.z, 0.0f };
		cw.chunk("AMBT", 1, amb, sizeof(amb));

		std::vector<rtx_point_light> pl(scene.point_light_count);
		for (int i = 0; i < scene.point_light_count; i++) { v3(pl[i].colour, scene.point_lights[i].colour); v3(pl[i].position, scene.point_lights[i].position); }
		cw.chunk("LPNT", (uint32_t)pl.size(), pl.data(), pl.size() * sizeof(rtx_point_light));
		std::vector<rtx_spot_light> sl(scene.spot_light_count);
		for (int i = 0; i < scene.spot_light_count; i++) {
			const SpotLight & s = scene.spot_lights[i];
			v3(sl[i].colour, s.colour); v3(sl[i].position, s.position); v3(sl[i].negative_direction, s.negative_direction);
			sl[i].inner_cutoff = s.inner_cutoff; sl[i].outer_cutoff = s.outer_cutoff;
		}
		cw.chunk("LSPT", (uint32_t)sl.size(), sl.data(), sl.size() * sizeof(rtx_spot_light));
		std::vector<rtx_directional_light> dl(scene.directional_light_count);
		for (int i = 0; i < scene.directional_light_count; i++) { v3(dl[i].colour, scene.directional_lights[i].colour); v3(dl[i].negative_direction, scene.directional_lights[i].negative_direction); }
		cw.chunk("LDIR", (uint32_t)dl.size(), dl.data(), dl.size() * sizeof(rtx_directional_light));

		// textures referenced by materials, in order of first use
		std::vector<const Texture *> textures;
		auto tex_id = [&](const Texture * t) -> int {
			if (!t) return -1;
			for (size_t i = 0; i < textures.size(); i++) if (textures[i] == t) return (int)i;
			textures.push_back(t); return (int)textures.size() - 1;
		};
		std::vector<rtx_material> mats(MaterialBuffer::material_count);
		for (int i = 0; i < MaterialBuffer::material_count; i++) {
			const Material & m = MaterialBuffer::materials[i];
			memset(&mats[i], 0, sizeof(rtx_material));
			v3(mats[i].diffuse, m.diffuse); mats[i].texture_id = tex_id(m.texture);
			v3(mats[i].reflection, m.reflection); v3(mats[i].transmittance, m.transmittance);
			mats[i].index_of_refraction = m.index_of_refraction;
		}
		cw.chunk("MATL", (uint32_t)mats.size(), mats.data(), mats.size() * sizeof(rtx_material));
		for (size_t t = 0; t < textures.size(); t++) {
			const Texture * tx = textures[t];
			rtx_texture_desc d; memset(&d, 0, sizeof(d));
			d.width = tx->width; d.height = tx->height; d.mipmapped = tx->mipmapped ? 1 : 0; d.mip_levels = tx->mip_levels;
			for (int l = 0; l < tx->mip_levels && l < RTX_MAX_MIP_LEVELS; l++) d.mip_offsets[l] = tx->mip_offsets[l];
			int64_t texels = (int64_t)tx->width * tx->height;
			if (tx->mipmapped) {
				// extent of the mip chain actually written by Texture::load (Texture.cpp:76-117)
				int lw = tx->width >> (tx->mip_levels - 1), lh = tx->height >> (tx->mip_levels - 1);
				texels = tx->mip_offsets[tx->mip_levels - 1] + (int64_t)std::max(lw, 1) * std::max(lh, 1);
			}
			cw.chunk("TEXH", (uint32_t)t, &d, sizeof(d));
			cw.chunk("TEXL", (uint32_t)t, tx->data, (uint64_t)texels * 12);
		}
		cw.chunk("SKYD", (uint32_t)scene.sky.size, scene.sky.data, (uint64_t)scene.sky.size * scene.sky.size * 12);

		// BLAS table: unique BottomLevelBVH pointers in order of first use
		std::vector<const BottomLevelBVH *> blas;
		auto blas_id = [&](const BottomLevelBVH * b) -> int {
			for (size_t i = 0; i < blas.size(); i++) if (blas[i] == b) return (int)i;
			blas.push_back(b); return (int)blas.size() - 1;
		};
		const TopLevelBVH & tl = scene.top_level_bvh;
		std::vector<rtx_instance> inst(tl.primitive_count);
		for (int i = 0; i < tl.primitive_count; i++) {
			memset(&inst[i], 0, sizeof(rtx_instance));
			inst[i].blas_id = blas_id(tl.primitives[i].bvh);
			memcpy(inst[i].world,     tl.primitives[i].transform.world_matrix.cells, 64);
			memcpy(inst[i].world_inv, tl.primitives[i].transform_inv.cells,          64);
		}
		for (size_t b = 0; b < blas.size(); b++) {
			int32_t hdr[4] = { blas[b]->node_count, blas[b]->index_count, blas[b]->material_offset, blas[b]->triangle_count };
			cw.chunk("BLSH", (uint32_t)b, hdr, sizeof(hdr));
			{
				std::vector<BVHNode> bn(blas[b]->nodes, blas[b]->nodes + blas[b]->node_count);
				if (bn.size() > 1) memset(&bn[1], 0, sizeof(BVHNode));
				cw.chunk("BLSN", (uint32_t)b, bn.data(), (uint64_t)blas[b]->node_count * sizeof(BVHNode));
			}
			cw.chunk("BLST", (uint32_t)b, blas[b]->triangles_hot,  (uint64_t)blas[b]->index_count * sizeof(BottomLevelBVH::TriangleHot));
			cw.chunk("BLSC", (uint32_t)b, blas[b]->triangles_cold, (uint64_t)blas[b]->index_count * sizeof(BottomLevelBVH::TriangleCold));
		}
		cw.chunk("INST", (uint32_t)inst.size(), inst.data(), inst.size() * sizeof(rtx_instance));
		{
			// node 1 is never written or read by the reference (BVHBuilders.h:20-21 starts at 2): zero it so fixtures are deterministic
			std::vector<BVHNode> tn(tl.nodes, tl.nodes + tl.node_count);
			if (tn.size() > 1) memset(&tn[1], 0, sizeof(BVHNode));
			cw.chunk("TLSN", (uint32_t)tl.node_count, tn.data(), (uint64_t)tl.node_count * sizeof(BVHNode));
		}
		cw.chunk("TLSI", (uint32_t)tl.leaf_count, tl.indices, (uint64_t)tl.leaf_count * 4);
		// instance positions: input of the TLAS rebuild (TopLevelBVH.cpp:32-45 sorts by transform.position)
		std::vector<float> ipos(tl.primitive_count * 7), iaabb(tl.primitive_count * 6);
		for (int i = 0; i < tl.primitive_count; i++) {
			const Transform & t = tl.primitives[i].transform;
			float * p = &ipos[7 * i]; p[0] = t.position.x; p[1] = t.position.y; p[2] = t.position.z; p[3] = t.rotation.x; p[4] = t.rotation.y; p[5] = t.rotation.z; p[6] = t.rotation.w;
			v3(&iaabb[6 * i], tl.primitives[i].aabb.min); v3(&iaabb[6 * i + 3], tl.primitives[i].aabb.max);
		}
		cw.chunk("IPOS", (uint32_t)tl.primitive_count, ipos.data(), ipos.size() * 4);
		cw.chunk("IAAB", (uint32_t)tl.primitive_count, iaabb.data(), iaabb.size() * 4);

		std::vector<rtx_sphere> sp(scene.spheres.primitive_count);
		for (int i = 0; i < scene.spheres.primitive_count; i++) {
			const Sphere & s = scene.spheres.primitives[i];
			v3(sp[i].center, s.transform.position); sp[i].radius_inv = s.radius_inv; sp[i].radius_squared = s.radius_squared; sp[i].material_id = s.material_id;
		}
		cw.chunk("SPHR", (uint32_t)sp.size(), sp.data(), sp.size() * sizeof(rtx_sphere));
		std::vector<rtx_plane> pn(scene.planes.primitive_count);
		for (int i = 0; i < scene.planes.primitive_count; i++) {
			const Plane & p = scene.planes.primitives[i];
			memset(&pn[i], 0, sizeof(rtx_plane));
			v3(pn[i].normal, p.world_normal); pn[i].distance = p.world_distance; v3(pn[i].u_axis, p.u_axis); v3(pn[i].v_axis, p.v_axis); pn[i].material_id = p.material_id;
		}
		cw.chunk("PLAN", (uint32_t)pn.size(), pn.data(), pn.size() * sizeof(rtx_plane));
	}

	auto dump = [&](const std::string & name, const void * data, size_t bytes) {
		FILE * f = fopen((outdir + "/" + name).c_str(), "wb"); fwrite(data, 1, bytes, f); fclose(f);
	};
	dump("rgb.f32", rgb.data(), rgb.size() * 4);
	dump("dist.f32", dist.data(), dist.size() * 4);
	dump("packed.u32", window.frame_buffer, (size_t)W * H * 4);

	// ---- texture probes: Texture::sample at seeded inputs (Texture.h:33-49) ------------------------
	for (size_t k = 0; k < probes.size(); k++) {
		const Texture * tx = Texture::load(probes[k].path.c_str());
		std::vector<float> io((size_t)probes[k].n * 9);
		unsigned s = probes[k].seed;
		auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) * (1.0f / 16777216.0f); };
		for (int i = 0; i < probes[k].n; i++) {
			float * r = &io[9 * (size_t)i];
			r[0] = rnd() * 4.0f - 2.0f; r[1] = rnd() * 4.0f - 2.0f;
			float scale = powf(2.0f, -10.0f * rnd());          // footprints from ~1 texel to the whole texture
			r[2] = (rnd() - 0.5f) * scale; r[3] = (rnd() - 0.5f) * scale * (rnd() < 0.3f ? 0.05f : 1.0f);
			r[4] = (rnd() - 0.5f) * scale; r[5] = (rnd() - 0.5f) * scale * (rnd() < 0.3f ? 0.05f : 1.0f);
			Vector3 c = tx->sample(r[0], r[1], r[2], r[3], r[4], r[5]);
			r[6] = c.x; r[7] = c.y; r[8] = c.z;
		}
		char name[64]; snprintf(name, sizeof(name), "texprobe%zu.f32", k);
		dump(name, io.data(), io.size() * 4);
	}

	// ---- texture probes at caller-supplied inputs (tests/texset.py): `texprobe_file <image> <inputs.f32>`, n x 6 floats in (s, t, ds_dx, ds_dy,
	// dt_dx, dt_dy), texprobe_file<k>.f32 out: n x 9 (the inputs, then Texture::sample's colour) --------------------------------------------
	for (size_t k = 0; k < file_probes.size(); k++) {
		const Texture * tx = Texture::load(file_probes[k].path.c_str());
		FILE * f = fopen(file_probes[k].inputs.c_str(), "rb");
		if (!f) { fprintf(stderr, "cannot read %s\n", file_probes[k].inputs.c_str()); return 2; }
		fseek(f, 0, SEEK_END); const long bytes = ftell(f); fseek(f, 0, SEEK_SET);
		const size_t n = (size_t)bytes / 24;
		std::vector<float> in(n * 6), io(n * 9);
		if (bytes % 24 != 0 || fread(in.data(), 4, in.size(), f) != in.size()) { fprintf(stderr, "%s: not n x 6 floats\n", file_probes[k].inputs.c_str()); return 2; }
		fclose(f);
		for (size_t i = 0; i < n; i++) {
			float * r = &io[9 * i];
			memcpy(r, &in[6 * i], 24);
			Vector3 c = tx->sample(r[0], r[1], r[2], r[3], r[4], r[5]);
			r[6] = c.x; r[7] = c.y; r[8] = c.z;
		}
		char name[64]; snprintf(name, sizeof(name), "texprobe_file%zu.f32", k);
		dump(name, io.data(), io.size() * 4);
	}

	// ---- unit probes: ONE reference function each at seeded inputs ----------------------------------------
	// unit_rays.f32    per ray 18 inputs (origin, direction, dO_dx, dO_dy, dD_dx, dD_dy) + Scene::trace_primitives' RayHit: hit, distance,
	//                  point, normal, material_id, u, v, ds_dx, ds_dy, dt_dx, dt_dy, dO_dx, dO_dy, dN_dx, dN_dy (27) + Scene::intersect_primitives
	//                  for max distances 3 and 1e30 (2): rays aimed at the scene's triangles, spheres and the plane, and some that miss
	// unit_aabb.f32    AABB::intersect: box min, max, ray origin, inverse direction, max distance (13) + mask (1)
	// unit_light.f32   Point / Spot / DirectionalLight::calc_lighting: normal, to_light, to_camera, distance_squared (10) + three colours (9)
	// unit_plot.f32    Window::plot: colour (3) + packed pixel bits (1)
	if (unit_n > 0) {
		unsigned s = unit_seed;
		auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) * (1.0f / 16777216.0f); };
		auto sym = [&](float a) { return (rnd() * 2.0f - 1.0f) * a; };
		std::vector<float> io((size_t)unit_n * 47);
		for (int i = 0; i < unit_n; i++) {
			float * r = &io[47 * (size_t)i];
			Vector3 o(sym(6.0f), rnd() * 6.0f, sym(6.0f) - 2.0f);
			Vector3 target(sym(5.0f), rnd() * 4.0f - 1.5f, sym(5.0f) + 4.0f);
			Vector3 d = Vector3::normalize(target - o);
			if (rnd() < 0.1f) d = Vector3(0.0f, rnd() < 0.5f ? -1.0f : 1.0f, 0.0f);        // axis-aligned: zero direction components
			Ray ray;
			ray.origin = SIMD_Vector3(o); ray.direction = SIMD_Vector3(d);
			Vector3 dox(sym(0.01f), sym(0.01f), sym(0.01f)), doy(sym(0.01f), sym(0.01f), sym(0.01f)), ddx(sym(0.002f), sym(0.002f), sym(0.002f)), ddy(sym(0.002f), sym(0.002f), sym(0.002f));
#if RAY_DIFFERENTIALS_ENABLED
			ray.dO_dx = SIMD_Vector3(dox); ray.dO_dy = SIMD_Vector3(doy); ray.dD_dx = SIMD_Vector3(ddx); ray.dD_dy = SIMD_Vector3(ddy);
#endif
			const Vector3 in[6] = { o, d, dox, doy, ddx, ddy };
			for (int k = 0; k < 6; k++) { r[3 * k] = in[k].x; r[3 * k + 1] = in[k].y; r[3 * k + 2] = in[k].z; }
			RayHit h;
			memset(&h, 0, sizeof(h)); h.hit = SIMD_float(0.0f); h.distance = SIMD_float(INFINITY);      // fields the reference leaves unwritten on a miss read 0 here
			scene.trace_primitives(ray, h);
			float * q = r + 18;
			q[0] = SIMD_float::all_false(h.hit) ? 0.0f : 1.0f; q[1] = h.distance[0];
			q[2] = h.point.x[0]; q[3] = h.point.y[0]; q[4] = h.point.z[0]; q[5] = h.normal.x[0]; q[6] = h.normal.y[0]; q[7] = h.normal.z[0];
			q[8] = (float)h.material_id[0]; q[9] = h.u[0]; q[10] = h.v[0];
#if RAY_DIFFERENTIALS_ENABLED
			q[11] = h.ds_dx[0]; q[12] = h.ds_dy[0]; q[13] = h.dt_dx[0]; q[14] = h.dt_dy[0];
			q[15] = h.dO_dx.x[0]; q[16] = h.dO_dx.y[0]; q[17] = h.dO_dx.z[0]; q[18] = h.dO_dy.x[0]; q[19] = h.dO_dy.y[0]; q[20] = h.dO_dy.z[0];
			q[21] = h.dN_dx.x[0]; q[22] = h.dN_dx.y[0]; q[23] = h.dN_dx.z[0]; q[24] = h.dN_dy.x[0]; q[25] = h.dN_dy.y[0]; q[26] = h.dN_dy.z[0];
#endif
			q[27] = SIMD_float::all_false(scene.intersect_primitives(ray, SIMD_float(3.0f))) ? 0.0f : 1.0f;
			q[28] = SIMD_float::all_false(scene.intersect_primitives(ray, SIMD_float(1e30f))) ? 0.0f : 1.0f;
		}
		dump("unit_rays.f32", io.data(), io.size() * 4);

		std::vector<float> ab((size_t)unit_n * 14);
		for (int i = 0; i < unit_n; i++) {
			float * r = &ab[14 * (size_t)i];
			AABB box;
			Vector3 c(sym(3.0f), sym(3.0f), sym(3.0f)), e(rnd() * 2.0f, rnd() * 2.0f, rnd() * 2.0f);
			if (rnd() < 0.2f) e.y = 0.0f;                                                  // flat boxes
			box.min = c - e; box.max = c + e;
			Vector3 o(sym(5.0f), sym(5.0f), sym(5.0f));
			if (rnd() < 0.2f) o.x = box.min.x;                                             // origin on a slab plane: 0 * inf when the direction component is 0
			Vector3 d = Vector3::normalize(Vector3(sym(1.0f), sym(1.0f), sym(1.0f)));
			if (rnd() < 0.6f) d = Vector3::normalize(c + Vector3(sym(1.2f) * e.x, sym(1.2f) * e.y, sym(1.2f) * e.z) - o);      // aimed at (or just past) the box
			if (rnd() < 0.3f) d.x = 0.0f;
			if (rnd() < 0.1f) d.z = -0.0f;
			Ray ray; ray.origin = SIMD_Vector3(o); ray.direction = SIMD_Vector3(d);
			SIMD_Vector3 inv = SIMD_Vector3::rcp(ray.direction);
			const float maxd = rnd() < 0.5f ? INFINITY : rnd() * 8.0f;
			SIMD_float m = box.intersect(ray, inv, SIMD_float(maxd));
			r[0] = box.min.x; r[1] = box.min.y; r[2] = box.min.z; r[3] = box.max.x; r[4] = box.max.y; r[5] = box.max.z;
			r[6] = o.x; r[7] = o.y; r[8] = o.z; r[9] = inv.x[0]; r[10] = inv.y[0]; r[11] = inv.z[0]; r[12] = maxd;
			r[13] = SIMD_float::all_false(m) ? 0.0f : 1.0f;
		}
		dump("unit_aabb.f32", ab.data(), ab.size() * 4);

		std::vector<float> li((size_t)unit_n * 19);
		PointLight pl(Vector3(20.0f, 30.0f, 26.0f), Vector3(0.0f));
		SpotLight  sl(Vector3(40.0f, 40.0f, 48.0f), Vector3(0.0f), Vector3::normalize(Vector3(-0.8f, -0.55f, 0.25f)), 50.0f, 70.0f);
		DirectionalLight dl(Vector3(0.9f, 0.8f, 0.7f), Vector3::normalize(Vector3(0.1f, -1.0f, 0.1f)));
		for (int i = 0; i < unit_n; i++) {
			float * r = &li[19 * (size_t)i];
			Vector3 n = Vector3::normalize(Vector3(sym(1.0f), sym(1.0f), sym(1.0f)));
			Vector3 tl = Vector3::normalize(Vector3(sym(1.0f), sym(1.0f), sym(1.0f)));
			if (rnd() < 0.3f) tl = Vector3::normalize(Vector3(0.8f, 0.55f, -0.25f) + Vector3(sym(0.4f), sym(0.4f), sym(0.4f)));      // inside / near the spot cone
			Vector3 tc = Vector3::normalize(Vector3(sym(1.0f), sym(1.0f), sym(1.0f)));
			const float d2 = 0.1f + rnd() * 50.0f;
			r[0] = n.x; r[1] = n.y; r[2] = n.z; r[3] = tl.x; r[4] = tl.y; r[5] = tl.z; r[6] = tc.x; r[7] = tc.y; r[8] = tc.z; r[9] = d2;
			SIMD_Vector3 a = pl.calc_lighting(SIMD_Vector3(n), SIMD_Vector3(tl), SIMD_Vector3(tc), SIMD_float(d2));
			SIMD_Vector3 b = sl.calc_lighting(SIMD_Vector3(n), SIMD_Vector3(tl), SIMD_Vector3(tc), SIMD_float(d2));
			SIMD_Vector3 c = dl.calc_lighting(SIMD_Vector3(n), SIMD_Vector3(tc));
			r[10] = a.x[0]; r[11] = a.y[0]; r[12] = a.z[0]; r[13] = b.x[0]; r[14] = b.y[0]; r[15] = b.z[0]; r[16] = c.x[0]; r[17] = c.y[0]; r[18] = c.z[0];
		}
		dump("unit_light.f32", li.data(), li.size() * 4);

		std::vector<float> pq((size_t)unit_n * 4);
		Window pw(1, 1, "plot");
		for (int i = 0; i < unit_n; i++) {
			float * r = &pq[4 * (size_t)i];
			const float k = rnd() < 0.2f ? 3.0f : 1.0f;
			r[0] = sym(0.6f) * k + 0.5f; r[1] = rnd() * k; r[2] = rnd() < 0.1f ? (float)(int)(rnd() * 255.0f) / 255.0f : rnd();
			pw.plot(0, 0, Vector3(r[0], r[1], r[2]));
			const unsigned px = pw.frame_buffer[0];
			memcpy(&r[3], &px, 4);
		}
		dump("unit_plot.f32", pq.data(), pq.size() * 4);
	}

	// ---- ray probes: caller-supplied rays (tests/rayset.py) through Scene::trace_primitives and Scene::intersect_primitives ---------
	// in:  <file> n records of RAYPROBE_IN floats: origin, direction, dO_dx, dO_dy, dD_dx, dD_dy (18), max distances (RAYPROBE_DIST)
	// out: rayprobe.f32 n records: the RayHit fields as unit_rays.f32 has them (27), then intersect_primitives at each max distance (RAYPROBE_DIST)
	if (rayprobe_n > 0) {
		enum { RAYPROBE_DIST = 7, RAYPROBE_IN = 18 + RAYPROBE_DIST, RAYPROBE_OUT = 27 + RAYPROBE_DIST };
		std::vector<float> in((size_t)rayprobe_n * RAYPROBE_IN), io((size_t)rayprobe_n * RAYPROBE_OUT);
		FILE * f = fopen(rayprobe_path.c_str(), "rb");
		if (!f || fread(in.data(), 4, in.size(), f) != in.size()) { fprintf(stderr, "cannot read %d rays from %s\n", rayprobe_n, rayprobe_path.c_str()); return 2; }
		fclose(f);
		for (int i = 0; i < rayprobe_n; i++) {
			const float * r = &in[(size_t)RAYPROBE_IN * i];
			float * q = &io[(size_t)RAYPROBE_OUT * i];
			const Vector3 o(r[0], r[1], r[2]), d(r[3], r[4], r[5]);
			Ray ray;
			ray.origin = SIMD_Vector3(o); ray.direction = SIMD_Vector3(d);
#if RAY_DIFFERENTIALS_ENABLED
			ray.dO_dx = SIMD_Vector3(Vector3(r[6], r[7], r[8]));    ray.dO_dy = SIMD_Vector3(Vector3(r[9], r[10], r[11]));
			ray.dD_dx = SIMD_Vector3(Vector3(r[12], r[13], r[14])); ray.dD_dy = SIMD_Vector3(Vector3(r[15], r[16], r[17]));
#endif
			RayHit h;
			memset(&h, 0, sizeof(h)); h.hit = SIMD_float(0.0f); h.distance = SIMD_float(INFINITY);
			scene.trace_primitives(ray, h);
			q[0] = SIMD_float::all_false(h.hit) ? 0.0f : 1.0f; q[1] = h.distance[0];
			q[2] = h.point.x[0]; q[3] = h.point.y[0]; q[4] = h.point.z[0]; q[5] = h.normal.x[0]; q[6] = h.normal.y[0]; q[7] = h.normal.z[0];
			q[8] = (float)h.material_id[0]; q[9] = h.u[0]; q[10] = h.v[0];
#if RAY_DIFFERENTIALS_ENABLED
			q[11] = h.ds_dx[0]; q[12] = h.ds_dy[0]; q[13] = h.dt_dx[0]; q[14] = h.dt_dy[0];
			q[15] = h.dO_dx.x[0]; q[16] = h.dO_dx.y[0]; q[17] = h.dO_dx.z[0]; q[18] = h.dO_dy.x[0]; q[19] = h.dO_dy.y[0]; q[20] = h.dO_dy.z[0];
			q[21] = h.dN_dx.x[0]; q[22] = h.dN_dx.y[0]; q[23] = h.dN_dx.z[0]; q[24] = h.dN_dy.x[0]; q[25] = h.dN_dy.y[0]; q[26] = h.dN_dy.z[0];
#endif
			for (int k = 0; k < RAYPROBE_DIST; k++)
				q[27 + k] = SIMD_float::all_false(scene.intersect_primitives(ray, SIMD_float(r[18 + k]))) ? 0.0f : 1.0f;
		}
		dump("rayprobe.f32", io.data(), io.size() * 4);
	}

	// ---- shade probes: caller-supplied primary rays (tests/shadeset.py) through Raytracer::bounce, each with a camera position of its own ------
	// in:  <file> n records of SHADEPROBE_IN floats: origin, direction, dO_dx, dO_dy, dD_dx, dD_dy (18), the camera position of this ray (3)
	// out: shadeprobe.f32 n records of SHADEPROBE_OUT floats: colour (3), distance (1), the primary, shadow, reflection and refraction ray
	//      counts of this ray's tree (4).  A record whose direction is all zero is no ray: its output record stays zero.
	// Scene::camera.position is written before each call (bounce reads it at Raytracer.cpp:152) and put back afterwards.
	if (shadeprobe_n > 0) {
		enum { SHADEPROBE_IN = 21, SHADEPROBE_OUT = 8 };
		std::vector<float> in((size_t)shadeprobe_n * SHADEPROBE_IN), io((size_t)shadeprobe_n * SHADEPROBE_OUT, 0.0f);
		FILE * f = fopen(shadeprobe_path.c_str(), "rb");
		if (!f || fread(in.data(), 4, in.size(), f) != in.size()) { fprintf(stderr, "cannot read %d rays from %s\n", shadeprobe_n, shadeprobe_path.c_str()); return 2; }
		fclose(f);
		const Vector3 camera_kept = scene.camera.position;
		for (int i = 0; i < shadeprobe_n; i++) {
			const float * r = &in[(size_t)SHADEPROBE_IN * i];
			float * q = &io[(size_t)SHADEPROBE_OUT * i];
			if (r[3] == 0.0f && r[4] == 0.0f && r[5] == 0.0f) continue;
			Ray ray;
			ray.origin = SIMD_Vector3(Vector3(r[0], r[1], r[2])); ray.direction = SIMD_Vector3(Vector3(r[3], r[4], r[5]));
#if RAY_DIFFERENTIALS_ENABLED
			ray.dO_dx = SIMD_Vector3(Vector3(r[6], r[7], r[8]));    ray.dO_dy = SIMD_Vector3(Vector3(r[9], r[10], r[11]));
			ray.dD_dx = SIMD_Vector3(Vector3(r[12], r[13], r[14])); ray.dD_dy = SIMD_Vector3(Vector3(r[15], r[16], r[17]));
#endif
			scene.camera.position = Vector3(r[18], r[19], r[20]);
			PerformanceStats st = { 0, 0, 0, 0 };
			st.num_primary_rays++;
			SIMD_float distance;
			SIMD_Vector3 colour = raytracer.bounce(ray, bounces, distance, st);
			q[0] = colour.x[0]; q[1] = colour.y[0]; q[2] = colour.z[0]; q[3] = distance[0];
			q[4] = (float)st.num_primary_rays; q[5] = (float)st.num_shadow_rays; q[6] = (float)st.num_reflection_rays; q[7] = (float)st.num_refraction_rays;
		}
		scene.camera.position = camera_kept;
		dump("shadeprobe.f32", io.data(), io.size() * 4);
	}

	{
		FILE * f = fopen((outdir + "/stats.json").c_str(), "w");
		fprintf(f, "{\"width\": %d, \"height\": %d, \"bounces\": %d, \"frames\": %d, \"delta\": %.9g,\n", W, H, bounces, frames, delta);
		fprintf(f, " \"mip_filter\": %d, \"texture_mode\": %d, \"scene_variant\": %d, \"simd_lane_size\": %d,\n", MIPMAP_FILTER, TEXTURE_SAMPLE_MODE, SCENE, SIMD_LANE_SIZE);
		fprintf(f, " \"primary\": %d, \"shadow\": %d, \"reflection\": %d, \"refraction\": %d,\n", stats_px.num_primary_rays, stats_px.num_shadow_rays, stats_px.num_reflection_rays, stats_px.num_refraction_rays);
		fprintf(f, " \"render_tile_pass\": %s, \"packed_mismatch\": %ld, \"render_tile_ms_1thread\": %.3f}\n", tiles_valid ? "true" : "false", packed_mismatch, tiles_valid ? best_ms : -1.0);
		fclose(f);
	}
	printf("refdump: %dx%d bounces=%d rays p=%d s=%d rl=%d rr=%d packed_mismatch=%ld tile_ms=%.2f\n", W, H, bounces,
	       stats_px.num_primary_rays, stats_px.num_shadow_rays, stats_px.num_reflection_rays, stats_px.num_refraction_rays, packed_mismatch, tiles_valid ? best_ms : -1.0);
	return packed_mismatch > 0 ? 3 : 0;
}
