#include <cmath>
#include "LightingECS.h"
#include "../RHI/Renderer.h"
#include "../GraphicsDriver/HIP/HipGraphicsDriver.h"

using namespace Sailor;
using namespace Sailor::RHI;

LightingECS::LightingECS(uint32_t capacity)
{
    auto driver = Renderer::GetDriver();
    m_lightsData = driver->CreateShaderBindings();
    driver->AddSsboToShaderBindings(m_lightsData, "light", sizeof(LightShaderData), capacity, 0, true); // LightingECS.cpp:44
}

size_t LightingECS::RegisterComponent(const LightData& data)
{
    m_components.push_back(data);
    return m_components.size() - 1;
}

// ---- which light slots one Tick uploads, as contiguous runs (the boundary contract of row L7: every run becomes ONE UpdateShaderBinding, and the HIP backend
// re-derives the prepared views of exactly those slots -- sailor_hip_prepare_lights(first, count)).  The rules are the reference's (ECS/LightingECS.cpp:93-192),
// restated around two small pieces of state instead of transliterated: the list of static-owner runs the loop steps over, and the run of packed
// records that is currently open.  oracle/oracle.py:lighting_tick_runs is an independent restatement; tests/test_host_cpu.py and
// tests/test_runtime_gpu.py::test_lighting_ecs_streams_dirty_runs_into_the_light_ssbo hold the two against each other slot for slot.
namespace {

// Slots whose owner is static are packed once -- on the pass that first meets them -- and stepped over from the next Tick on, dirty or not.  The list holds them
// as (first slot, length) runs in slot order; `passed` counts the runs the current pass has stepped over or opened.
struct StaticRuns {
    std::vector<std::pair<uint32_t, uint32_t>>& runs;
    uint32_t passed = 0;

    // (:95-103) if the next run starts at `index`, jump behind it; false = the jump left the array.  (ONE run per loop step, as the reference: two runs that touch
    // are stepped over in two steps.)
    bool StepOver(size_t& index, size_t num)
    {
        if (passed < runs.size() && index == runs[passed].first) {
            index += runs[passed].second;
            if (index >= num) return false;
            passed++;
        }
        return true;
    }

    // (:108-146) slot `index` has a static owner and was not stepped over: it extends the run just passed when it follows it directly, opens a run of its own in
    // the gap between two later runs, or is appended.  (The gap's lower bound uses the length of the run just passed for EVERY gap -- the reference's arithmetic,
    // kept because it decides which later Ticks step over what.)
    void Note(size_t index)
    {
        if (passed > 0) {
            std::pair<uint32_t, uint32_t>& last = runs[passed - 1];
            if (index == (size_t)last.first + last.second) { last.second++; return; }
            for (size_t i = passed - 1; i + 1 < runs.size(); i++) {
                const uint32_t gapBegin = runs[i].first + last.second, gapEnd = runs[i + 1].first;
                if (index > gapBegin && index < gapEnd) {
                    runs.insert(runs.begin() + (long)(i + 1), std::make_pair((uint32_t)index, 1u));
                    passed++;
                    return;
                }
            }
        }
        runs.emplace_back((uint32_t)index, 1u);
        passed++;
    }
};

// The run of freshly packed records that is open: closed -- one copy -- when a slot that needs no upload follows it, or at the last slot.
struct OpenRun {
    std::vector<LightUploadRun>& out;
    size_t start = 0, count = 0;
    bool open = false;
    void Add(size_t index) { if (!open) { open = true; start = index; } count++; }
    void Close() { open = false; }
    void FlushIf(bool atEnd) { if ((!open || atEnd) && count > 0) { out.push_back({ start, count }); count = 0; } }
};

} // namespace

// Two consequences of where the reference's `continue` sits (:148-149), reproduced because they decide what reaches the SSBO: an INACTIVE slot neither closes nor
// flushes the open run -- a dirty run that continues behind it is written as one copy whose later records land one slot early -- and a run still open when the
// last slot is inactive (or when the static runs step past the end) is never written although its lights were marked clean.
std::vector<LightUploadRun> LightingECS::CollectDirtyRuns(std::vector<LightData>& components, std::vector<std::pair<uint32_t, uint32_t>>& skipList,
                                                          std::vector<LightShaderData>& records)
{
    std::vector<LightUploadRun> runs;
    StaticRuns statics { skipList };
    OpenRun run { runs };
    const size_t num = components.size();
    for (size_t index = 0; index < num; index++) {
        if (!statics.StepOver(index, num)) break;
        LightData& data = components[index];
        if (data.m_ownerMobility == EMobilityType::Static) statics.Note(index);
        if (!data.m_bIsActive) continue;
        const bool upload = data.m_bIsDirty || data.m_frameLastChange < data.m_ownerFrameLastChange; // (:152) dirty, or the owner moved after the last packing
        if (upload) {
            LightShaderData shaderData;
            sailor_host_pack_light((uint32_t)data.m_type, (uint32_t)data.m_shadowType, data.m_worldPosition, data.m_direction, data.m_intensity,
                                   data.m_attenuation, data.m_cutOff, data.m_bounds, &shaderData); // (:162-172)
            records.push_back(shaderData);
            run.Add(index);
            data.m_frameLastChange = data.m_ownerFrameLastChange; // (:174)
            data.m_bIsDirty = false;
        } else run.Close();
        run.FlushIf(index == num - 1); // (:182-191) one copy per run
    }
    records.resize(records.size() - run.count); // a run that was never flushed is never written
    return runs;
}

void LightingECS::Tick(RHICommandListPtr cmdList)
{
    auto binding = m_lightsData->GetOrAddShaderBinding("light");
    std::vector<LightShaderData> records;
    m_lastUploads = CollectDirtyRuns(m_components, m_skipList, records);
    size_t at = 0;
    for (const LightUploadRun& run : m_lastUploads) {
        Renderer::GetDriverCommands()->UpdateShaderBinding(cmdList, binding, records.data() + at, sizeof(LightShaderData) * run.m_count,
                                                           binding->GetBufferOffset() + sizeof(LightShaderData) * run.m_startIndex);
        at += run.m_count;
    }
    m_packedCount = m_components.size(); // FillLightingData: m_totalNumLights counts every slot, active or not (:404)
}

void LightingECS::SetPacked(RHICommandListPtr cmdList, const LightShaderData* records, size_t count)
{
    auto binding = m_lightsData->GetOrAddShaderBinding("light");
    if (count) Renderer::GetDriverCommands()->UpdateShaderBinding(cmdList, binding, records, sizeof(LightShaderData) * count, 0);
    m_packedCount = count;
}

void LightingECS::SetShadowMaps(const TVector<RHITexturePtr>& maps, const float* lightsMatrices64)
{
    auto driver = Renderer::GetDriver();
    driver->AddSamplerToShaderBindings(m_lightsData, "shadowMaps", maps, 8);                                               // LightingECS.cpp:71
    auto b = driver->AddBufferToShaderBindings(m_lightsData, "lightsMatrices", 256, 6, EShaderBindingType::UniformBuffer); // :74 (SSBO there)
    memcpy(b->m_hostCopy.data(), lightsMatrices64, 256);
}

void LightingECS::FillLightingData(RHISceneViewSnapshot& snapshot) const
{
    snapshot.m_totalNumLights = (uint32_t)m_packedCount; // includes inactive slots in the reference (LightingECS.cpp:404)
    snapshot.m_rhiLightsData = m_lightsData;
}

// ---- the cascades: LightingECS::PrepareCSMPasses (ECS/LightingECS.cpp:262-371) and the shadow half of FillLightingData (:373-406) --------------------------
LightingECS::~LightingECS() { sailor_host_csm_snapshots_destroy(m_csmSnapshots); }

void LightingECS::SetCasterData(const CsmCasterData* casters)
{
    m_bHasCasters = casters != nullptr;
    m_casters = casters ? *casters : CsmCasterData();
}

TVector<CsmPassPlan> LightingECS::PlanLightPasses(SailorCsmSnapshots* snapshots, uint32_t firstSnapshot, uint32_t alreadyPlacedPasses, uint32_t numInstances,
                                                  const uint64_t* overlapMasks, EShadowType lightShadowType, const uint64_t* lastChangedFrame,
                                                  const SailorCsmView* view, const uint64_t* castShadows)
{
    const size_t words = ((size_t)numInstances + 63) / 64;
    uint32_t shadowTypes[NumCascades], render[NumCascades];
    for (uint32_t k = 0; k < NumCascades; k++) shadowTypes[k] = (uint32_t)(k > 0 ? EShadowType::PCF : lightShadowType); // :303 for EVSM only the 1st cascade is EVSM
    TVector<uint64_t> finalMasks(NumCascades * words);
    TVector<CsmPassPlan> plans;
    // the removal (:310-327), the snapshot comparison and the snapshots' update (:334-366)
    if (sailor_host_csm_plan_passes(snapshots, firstSnapshot, NumCascades, numInstances, overlapMasks, shadowTypes, lastChangedFrame, view, render,
                                    finalMasks.data()) != SAILOR_HIP_OK)
        return plans;
    for (uint32_t k = 0; k < NumCascades; k++) {
        if (!render[k]) continue; // :349-353 an equal snapshot: no pass
        CsmPassPlan plan;
        plan.m_cascade = k;
        plan.m_shadowType = (EShadowType)shadowTypes[k];
        if (k > 0) { // :305-332, with bCascadeAdded[z] = render[z] ? shadowTypes[z] : None
            TVector<uint64_t> left(overlapMasks + (size_t)k * words, overlapMasks + (size_t)(k + 1) * words);
            int32_t shift = -1;
            for (uint32_t z = 0; z < k; z++) {
                if (render[z]) shift++;                                   // :310-313
                if (!render[z] || shadowTypes[z] != shadowTypes[k]) continue; // :315-318
                bool removed = false;                                     // :321-324 RemoveAll(frustums[z].OverlapsAABB)
                for (size_t w = 0; w < words; w++) {
                    const uint64_t overlapZ = overlapMasks[(size_t)z * words + w];
                    removed = removed || (left[w] & overlapZ) != 0;
                    left[w] &= ~overlapZ;
                }
                if (removed) plan.m_internalCommandsList.push_back(alreadyPlacedPasses + (uint32_t)shift); // :327-330
            }
        }
        plan.m_casterMask.assign(finalMasks.begin() + (long)(k * words), finalMasks.begin() + (long)((k + 1) * words));
        if (castShadows) for (size_t w = 0; w < words; w++) plan.m_casterMask[w] &= castShadows[w]; // ShadowPrepassNode.cpp:110
        if (words && (numInstances & 63)) plan.m_casterMask[words - 1] &= (1ull << (numInstances & 63)) - 1ull; // no bits past the last instance
        plans.push_back(std::move(plan));
    }
    return plans;
}

uint32_t LightingECS::CountBatchRuns(const TVector<uint64_t>& mask, const TVector<RHISceneBatch>& batches, TVector<RHIShadowBatchRun>& outRuns)
{
    auto popcount_range = [&](uint64_t begin, uint64_t end) {
        uint32_t n = 0;
        for (uint64_t w = begin / 64; w * 64 < end && w < mask.size(); w++) {
            uint64_t v = mask[(size_t)w];
            if (w * 64 < begin) v &= ~0ull << (begin - w * 64);
            if (end - w * 64 < 64) v &= (1ull << (end - w * 64)) - 1ull;
            n += (uint32_t)__builtin_popcountll(v);
        }
        return n;
    };
    outRuns.assign(batches.size(), RHIShadowBatchRun());
    uint32_t total = 0;
    for (size_t b = 0; b < batches.size(); b++) {
        outRuns[b].m_offset = total;
        outRuns[b].m_count = popcount_range(batches[b].m_firstInstance, (uint64_t)batches[b].m_firstInstance + batches[b].m_instanceCount);
        total += outRuns[b].m_count;
    }
    return total;
}

int LightingECS::EnsureCsmShadowMaps(EShadowType firstCascadeType)
{
    auto driver = Renderer::GetDriver();
    bool create = m_csmShadowMaps.size() != NumCascades || m_csmFirstCascadeType != firstCascadeType;
    for (uint32_t k = 0; k < NumCascades && !create; k++)
        create = m_csmShadowMaps[k]->GetExtent().x != m_casters.m_resolutions[k].x || m_csmShadowMaps[k]->GetExtent().y != m_casters.m_resolutions[k].y;
    if (create) { // :53-63: cascade 0 in the EVSM format when the light is EVSM, the others (and a PCF light's cascade 0) in ShadowMapFormat
        m_csmShadowMaps.clear();
        for (uint32_t k = 0; k < NumCascades; k++) {
            auto map = driver->CreateRenderTarget(m_casters.m_resolutions[k], 1, k == 0 && firstCascadeType == EShadowType::EVSM ? EFormat::R32G32B32A32_SFLOAT : EFormat::R16_SFLOAT);
            if (!map) { m_csmShadowMaps.clear(); return SAILOR_HIP_ERR_OUT_OF_MEMORY; }
            m_csmShadowMaps.push_back(map);
        }
        m_csmFirstCascadeType = firstCascadeType;
        sailor_host_csm_snapshots_destroy(m_csmSnapshots); // new maps hold nothing: every cascade is rendered again
        m_csmSnapshots = nullptr;
    }
    // :65-75 `shadowMaps` (binding 8), `lightsMatrices` (6), `shadowIndices` (7) of the lights set
    auto maps = m_lightsData->Find("shadowMaps");
    if (create || !maps || maps->m_textures.size() < NumCascades || maps->m_textures[0].GetRawPtr() != m_csmShadowMaps[0].GetRawPtr()) {
        driver->AddSamplerToShaderBindings(m_lightsData, "shadowMaps", m_csmShadowMaps, 8);
        if (!m_lightsData->Find("lightsMatrices")) driver->AddBufferToShaderBindings(m_lightsData, "lightsMatrices", 64 * NumCascades, 6, EShaderBindingType::UniformBuffer); // (SSBO there)
        if (!m_lightsData->Find("shadowIndices")) driver->AddSsboToShaderBindings(m_lightsData, "shadowIndices", sizeof(uint32_t), MaxShadowsInView, 7);
    }
    return SAILOR_HIP_OK;
}

// glm::quat_cast of the rotation part of a world matrix (the camera's Math::Transform reaches the mirror as its matrix): (x, y, z, w)
static void quat_from_matrix(const float* m, float* q)
{
    const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[4], m11 = m[5], m12 = m[6], m20 = m[8], m21 = m[9], m22 = m[10]; // m[c][r] = m[4 c + r]
    const float fourXSquaredMinus1 = m00 - m11 - m22, fourYSquaredMinus1 = m11 - m00 - m22, fourZSquaredMinus1 = m22 - m00 - m11, fourWSquaredMinus1 = m00 + m11 + m22;
    int biggestIndex = 0;
    float fourBiggestSquaredMinus1 = fourWSquaredMinus1;
    if (fourXSquaredMinus1 > fourBiggestSquaredMinus1) { fourBiggestSquaredMinus1 = fourXSquaredMinus1; biggestIndex = 1; }
    if (fourYSquaredMinus1 > fourBiggestSquaredMinus1) { fourBiggestSquaredMinus1 = fourYSquaredMinus1; biggestIndex = 2; }
    if (fourZSquaredMinus1 > fourBiggestSquaredMinus1) { fourBiggestSquaredMinus1 = fourZSquaredMinus1; biggestIndex = 3; }
    const float biggestVal = std::sqrt(fourBiggestSquaredMinus1 + 1.0f) * 0.5f, mult = 0.25f / biggestVal;
    switch (biggestIndex) {
    case 0: q[3] = biggestVal; q[0] = (m12 - m21) * mult; q[1] = (m20 - m02) * mult; q[2] = (m01 - m10) * mult; break;
    case 1: q[3] = (m12 - m21) * mult; q[0] = biggestVal; q[1] = (m01 + m10) * mult; q[2] = (m20 + m02) * mult; break;
    case 2: q[3] = (m20 - m02) * mult; q[0] = (m01 + m10) * mult; q[1] = biggestVal; q[2] = (m12 + m21) * mult; break;
    default: q[3] = (m01 - m10) * mult; q[0] = (m20 + m02) * mult; q[1] = (m12 + m21) * mult; q[2] = biggestVal; break;
    }
}

int LightingECS::FillShadowPasses(RHISceneViewSnapshot& snapshot)
{
    snapshot.m_shadowMapsToUpdate.clear();
    if (!m_bHasCasters) return SAILOR_HIP_OK;
    auto* hip = dynamic_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    if (!hip || !m_casters.m_worldAabb) return SAILOR_HIP_ERR_UNSUPPORTED;
    const uint32_t numInstances = m_casters.m_numInstances;
    const size_t words = ((size_t)numInstances + 63) / 64;
    if (m_casters.m_lastChangedFrame.size() < numInstances || (!m_casters.m_castShadows.empty() && m_casters.m_castShadows.size() < words) ||
        m_casters.m_worldAabb->m_size < (size_t)numInstances * sizeof(SailorAABB))
        return SAILOR_HIP_ERR_INVALID_ARGUMENT;
    const CameraData& camera = snapshot.m_camera;
    float planes[24];
    sailor_host_extract_frustum_planes(camera.m_world, camera.m_aspect, camera.m_fov, camera.m_zNear, camera.m_zFar, planes, nullptr); // :381-382

    // GetLightsInFrustum (:209-260, :389): the directional lights that cast shadows, in component order
    const size_t numLights = m_components.size();
    std::vector<uint32_t> types(numLights), shadowTypes(numLights), directional(numLights), point(numLights), spot(numLights);
    std::vector<uint8_t> active(numLights);
    std::vector<float> positions(3 * numLights), bounds(3 * numLights), pointDistance(numLights), spotDistance(numLights);
    for (size_t i = 0; i < numLights; i++) {
        const LightData& light = m_components[i];
        types[i] = (uint32_t)light.m_type; shadowTypes[i] = (uint32_t)light.m_shadowType; active[i] = light.m_bIsActive ? 1 : 0;
        memcpy(&positions[3 * i], light.m_worldPosition, 12); memcpy(&bounds[3 * i], light.m_bounds, 12);
    }
    uint32_t numDirectional = 0, numPoint = 0, numSpot = 0;
    if (numLights) {
        const int st = sailor_host_lights_in_frustum(planes, camera.m_world + 12, (uint32_t)numLights, types.data(), shadowTypes.data(), active.data(), positions.data(),
                                                     bounds.data(), directional.data(), &numDirectional, point.data(), pointDistance.data(), &numPoint, spot.data(),
                                                     spotDistance.data(), &numSpot);
        if (st != SAILOR_HIP_OK) return st;
    }
    if (numDirectional == 0) { // (:392-397 with no directional light: the snapshots are dropped)
        sailor_host_csm_snapshots_destroy(m_csmSnapshots);
        m_csmSnapshots = nullptr;
        return SAILOR_HIP_OK;
    }
    // the one set of cascade maps belongs to the first light (:297 m_csmShadowMaps[k]); its type decides cascade 0's format
    int st = EnsureCsmShadowMaps(m_components[directional[0]].m_shadowType);
    if (st != SAILOR_HIP_OK) return st;
    // :391-397 the snapshots are kept only while their number fits the view
    const uint32_t numCsmSnapshots = numDirectional * NumCascades;
    if (m_csmSnapshots && sailor_host_csm_snapshots_count(m_csmSnapshots) != numCsmSnapshots) { sailor_host_csm_snapshots_destroy(m_csmSnapshots); m_csmSnapshots = nullptr; }
    if (!m_csmSnapshots) m_csmSnapshots = sailor_host_csm_snapshots_create();
    if (!m_csmSnapshots) return SAILOR_HIP_ERR_OUT_OF_MEMORY;
    if (!m_csmMasks || m_csmMasks->m_size < NumCascades * words * 8 + 8) m_csmMasks = hip->CreateBuffer(NumCascades * words * 8 + 8);
    if (!m_csmMasks) return SAILOR_HIP_ERR_OUT_OF_MEMORY;

    SailorCsmView view {};
    for (int i = 0; i < 3; i++) view.cameraPosition[i] = camera.m_world[12 + i];
    view.cameraPosition[3] = 1.0f;
    quat_from_matrix(camera.m_world, view.cameraRotation);
    std::vector<uint64_t> overlap(NumCascades * words);
    uint32_t snapshotIndex = 0;
    for (uint32_t d = 0; d < numDirectional; d++) { // :274
        const LightData& light = m_components[directional[d]];
        SailorTransform lightTransform {};
        memcpy(lightTransform.position, light.m_worldPosition, 12); lightTransform.position[3] = 0.0f;
        memcpy(lightTransform.rotation, light.m_ownerRotation, 16);
        for (int i = 0; i < 4; i++) lightTransform.scale[i] = 1.0f;
        float lightWorld[16], lightView[16], lightsMatrices[16 * NumCascades], cascadePlanes[24 * NumCascades];
        sailor_host_transform_matrix(&lightTransform, lightWorld);
        sailor_host_mat4_inverse(lightWorld, lightView);                                                                              // :227
        sailor_host_csm_matrices(lightView, camera.m_world, camera.m_aspect, camera.m_fov, camera.m_zNear, camera.m_zFar, lightsMatrices); // :276-281, :292
        for (uint32_t k = 0; k < NumCascades; k++) sailor_host_extract_frustum_planes_matrix(lightsMatrices + 16 * k, cascadePlanes + 24 * k, nullptr); // :293
        // :296 cascade.m_meshList = sceneView->TraceScene(frustums[k], true), every cascade at once, then to the host (this waits for the stream)
        if (numInstances) {
            const SailorSceneTrace trace = { m_casters.m_traceMode, m_casters.m_rootSize, nullptr };
            st = m_casters.m_traceMode == SAILOR_TRACE_FLAT_FLOAT_BOXES
                     ? sailor_hip_csm_caster_masks(hip->GetContext(), numInstances, (const SailorAABB*)m_casters.m_worldAabb->m_hip.m_devicePtr, cascadePlanes, NumCascades,
                                                   (uint64_t*)m_csmMasks->m_hip.m_devicePtr)
                     : sailor_hip_csm_caster_masks_traced(hip->GetContext(), numInstances, (const SailorAABB*)m_casters.m_worldAabb->m_hip.m_devicePtr, cascadePlanes,
                                                          NumCascades, (uint64_t*)m_csmMasks->m_hip.m_devicePtr, &trace);
            if (st == SAILOR_HIP_OK) st = sailor_hip_buffer_download(hip->GetContext(), overlap.data(), m_csmMasks->m_hip.m_devicePtr, 0, NumCascades * words * 8);
            if (st != SAILOR_HIP_OK) return st;
        }
        view.componentIndex = directional[d];
        memcpy(view.lightPosition, lightTransform.position, 16);
        memcpy(view.lightRotation, lightTransform.rotation, 16);
        const uint32_t alreadyPlacedPasses = (uint32_t)snapshot.m_shadowMapsToUpdate.size(); // :286
        const auto plans = PlanLightPasses(m_csmSnapshots, snapshotIndex, alreadyPlacedPasses, numInstances, overlap.data(), light.m_shadowType,
                                           m_casters.m_lastChangedFrame.data(), &view, m_casters.m_castShadows.empty() ? nullptr : m_casters.m_castShadows.data());
        for (const CsmPassPlan& plan : plans) { // :295-303, :365
            RHIUpdateShadowMapCommand cascade;
            cascade.m_shadowMap = m_csmShadowMaps[plan.m_cascade];
            memcpy(cascade.m_lightMatrix, lightsMatrices + 16 * plan.m_cascade, 64);
            cascade.m_lighMatrixIndex = plan.m_cascade;
            cascade.m_blurRadius[0] = ShadowCascadeBlur[plan.m_cascade][0]; cascade.m_blurRadius[1] = ShadowCascadeBlur[plan.m_cascade][1];
            cascade.m_shadowType = plan.m_shadowType;
            cascade.m_internalCommandsList = plan.m_internalCommandsList;
            cascade.m_casterMask = plan.m_casterMask;
            cascade.m_numCasters = CountBatchRuns(cascade.m_casterMask, snapshot.m_batches, cascade.m_batchRuns);
            snapshot.m_shadowMapsToUpdate.push_back(std::move(cascade));
        }
        snapshotIndex += NumCascades;
    }
    return SAILOR_HIP_OK;
}

EcsSweepSystem::EcsSweepSystem(const SailorTransform* transforms, const uint32_t* parent, const SailorAABB* localAabb, uint32_t count,
                               const uint32_t* levelOffsets, uint32_t numLevels)
    : m_count(count), m_levelOffsets(levelOffsets, levelOffsets + numLevels + 1)
{
    auto driver = Renderer::GetDriver();
    auto cmds = Renderer::GetDriverCommands();
    auto cmd = driver->CreateCommandList();
    m_transforms = driver->CreateBuffer(sizeof(SailorTransform) * (size_t)count);
    m_parent = driver->CreateBuffer(4 * (size_t)count);
    m_localAabb = driver->CreateBuffer(sizeof(SailorAABB) * (size_t)count);
    m_world = driver->CreateBuffer(64 * (size_t)count);
    m_worldAabb = driver->CreateBuffer(sizeof(SailorAABB) * (size_t)count);
    m_visibility = driver->CreateBuffer(8 * (((size_t)count + 63) / 64));
    cmds->UpdateBuffer(cmd, m_transforms, transforms, sizeof(SailorTransform) * (size_t)count);
    cmds->UpdateBuffer(cmd, m_parent, parent, 4 * (size_t)count);
    cmds->UpdateBuffer(cmd, m_localAabb, localAabb, sizeof(SailorAABB) * (size_t)count);
    driver->SubmitCommandList(cmd);
}

void EcsSweepSystem::SetTraceMode(uint32_t mode, uint32_t rootSize)
{
    m_traceMode = mode;
    m_rootSize = rootSize;
    if (mode != SAILOR_TRACE_OCTREE_INT_BOXES || m_inserted) return;
    // cleared once: the sweep writes the entities' bits only, so the bits past m_count in the last word stay what the buffer held
    auto driver = Renderer::GetDriver();
    const size_t bytes = 8 * (((size_t)m_count + 63) / 64);
    m_inserted = driver->CreateBuffer(bytes);
    const std::vector<uint8_t> zeros(bytes, 0);
    auto cmd = driver->CreateCommandList();
    Renderer::GetDriverCommands()->UpdateBuffer(cmd, m_inserted, zeros.data(), bytes);
    driver->SubmitCommandList(cmd);
}

int EcsSweepSystem::Tick(const float* cameraWorld, float aspect, float fovDegrees, float zNear, float zFar)
{
    float planes[24];
    sailor_host_extract_frustum_planes(cameraWorld, aspect, fovDegrees, zNear, zFar, planes, nullptr); // RHI/SceneView.cpp:158
    auto* hip = dynamic_cast<GraphicsDriver::HIP::HipGraphicsDriver*>(Renderer::GetDriver());
    if (!hip) return SAILOR_HIP_ERR_UNSUPPORTED;
    if (m_traceMode != SAILOR_TRACE_FLAT_FLOAT_BOXES) {
        const SailorSceneTrace trace = { m_traceMode, m_rootSize, m_inserted ? (uint64_t*)m_inserted->m_hip.m_devicePtr : nullptr };
        return sailor_hip_ecs_sweep_traced(hip->GetContext(), m_count, (const SailorTransform*)m_transforms->m_hip.m_devicePtr,
                                           (const uint32_t*)m_parent->m_hip.m_devicePtr, m_levelOffsets.data(), (uint32_t)m_levelOffsets.size() - 1,
                                           (const SailorAABB*)m_localAabb->m_hip.m_devicePtr, planes, (float*)m_world->m_hip.m_devicePtr,
                                           (SailorAABB*)m_worldAabb->m_hip.m_devicePtr, (uint64_t*)m_visibility->m_hip.m_devicePtr, 0u, m_count, &trace);
    }
    return sailor_hip_ecs_sweep(hip->GetContext(), m_count, (const SailorTransform*)m_transforms->m_hip.m_devicePtr, (const uint32_t*)m_parent->m_hip.m_devicePtr,
                                m_levelOffsets.data(), (uint32_t)m_levelOffsets.size() - 1, (const SailorAABB*)m_localAabb->m_hip.m_devicePtr, planes,
                                (float*)m_world->m_hip.m_devicePtr, (SailorAABB*)m_worldAabb->m_hip.m_devicePtr, (uint64_t*)m_visibility->m_hip.m_devicePtr);
}
