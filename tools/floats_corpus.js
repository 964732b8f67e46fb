'use strict'
// Non-integer-number corpus for the JSON calls of a context opened with YGM_F_FLOATS (test tooling): states that hold
// floats, with what yjs 13.5.16 (the image's bundle, tools/yjs_bundle.js) and y-prosemirror's restated function give
// for them -- computed by the existing corpus tools with their refusal tables switched to the flag's (setFloats) -- and
// beside each the status a context WITHOUT the flag gives (the same tools, switched back), so that one fixture pins
// both behaviours.
//   tojson  { note, state, asks: [[nameHex, kind, status, jsonHex, statusWithoutFlag], ...] }       ygm_tojson_v1
//           the two float families of tojson_corpus.js's refusals, a float beside a BigInt, Maps and Arrays of every
//           edge value of tools/dtoa_corpus.js (bare, and nested in objects and arrays inside an Any), then
//           tojson_corpus.js's seeded random sessions with `floaty` forced on
//   json    { note, state, asks: [[nameHex, status, jsonHex, statusWithoutFlag], ...] }             ygm_json_v1
//           the three float families of json_corpus.js's refusals, every edge value as an attribute, floats in marks
//           and embeds, and a state whose only float is a 17-digit one inside an embed (status 3 with the flag too:
//           the state's parse calls the text not canonical)
//   fields  { note, state, asks: [[fields, status, jsonHex, statusWithoutFlag], ...] }              ygm_json_fields_v1
//           a float in the second field: refused without the flag only when that field is reached
//   node tools/floats_corpus.js <out.json.gz>
const fs = require('fs')
const path = require('path')
const zlib = require('zlib')
const Y = require(path.join(__dirname, 'yjs_bundle.js')).load()
const TJ = require(path.join(__dirname, 'tojson_corpus.js'))
const PJ = require(path.join(__dirname, 'json_corpus.js'))
const PF = require(path.join(__dirname, 'json_fields_corpus.js'))
const { edgeDoubles } = require(path.join(__dirname, 'dtoa_corpus.js'))

const SESSIONS = 120
const { MAP, ARRAY, TEXT } = TJ
const hex = s => Buffer.from(s, 'utf8').toString('hex')
const floats = on => { TJ.setFloats(on); PJ.setFloats(on) }
// the edge values an Any can carry through yjs 13.5.16 (its lib0 writes an integer below -2^31 as a varint that no
// document writes back: the state's parse refuses such a state whatever is asked)
const EDGES = edgeDoubles().filter(x => !(Number.isInteger(x) && x < -2147483647))

function tojsonEntry (note, state, asks) {
  floats(true)
  const on = asks.map(([n, k]) => TJ.ask(state, n, k))
  floats(false)
  const off = asks.map(([n, k]) => TJ.ask(state, n, k))
  return { note, state: Buffer.from(state).toString('hex'), asks: on.map((r, i) => [r[0], r[1], r[2], hex(r[3]), off[i][2]]) }
}
function jsonEntry (note, state) {
  floats(true)
  const on = PJ.rootsOf(state)
  floats(false)
  const off = PJ.rootsOf(state)
  return { note, state: Buffer.from(state).toString('hex'), asks: on.map((r, i) => [r[0], r[1], hex(r[2]), off[i][1]]) }
}
function fieldsEntry (note, state, lists) {
  floats(true)
  const on = lists.map(l => PF.fieldsOf(state, l))
  floats(false)
  const off = lists.map(l => PF.fieldsOf(state, l))
  return { note, state: Buffer.from(state).toString('hex'), asks: lists.map((l, i) => [l === null ? null : l.map(hex), on[i][0], hex(on[i][1]), off[i][0]]) }
}
const doc = (id, f) => { const d = new Y.Doc(); d.clientID = id; f(d); return Y.encodeStateAsUpdate(d) }
const frag = d => d.getXmlFragment('default')
const para = (parent, at, s) => { const e = new Y.XmlElement('paragraph'); parent.insert(at, [e]); const t = new Y.XmlText(); e.insert(0, [t]); if (s) t.insert(0, s); return e }

function tojsonPart () {
  const out = []
  for (const e of TJ.edges()) {
    if (e.note === 'refused: a finite non-integer number' || e.note === 'refused: an integer above 2^53') {
      out.push(tojsonEntry(e.note, Buffer.from(e.state, 'hex'), e.asks.map(r => [Buffer.from(r[0], 'hex').toString('utf8'), r[1]])))
    }
  }
  out.push(tojsonEntry('a float before a BigInt, and a float after a Uint8Array', doc(401, d => {
    d.getMap('m').set('w', 1.5); d.getMap('m').set('big', { n: BigInt(5) })
    d.getArray('a').push([{ bin: new Uint8Array([1]) }, 2.5])
  }), [['m', MAP], ['a', ARRAY]]))
  out.push(tojsonEntry('every edge value, bare, in a Map and an Array', doc(402, d => {
    EDGES.forEach((x, i) => d.getMap('m').set('v' + i, x))
    d.getArray('a').push(EDGES)
  }), [['m', MAP], ['a', ARRAY]]))
  out.push(tojsonEntry('every edge value nested in objects and arrays inside an Any', doc(403, d => {
    const o = []   // (objects of 32 keys: the state's parse tracks at most 64 keys per object)
    EDGES.forEach((x, i) => { if (i % 32 === 0) o.push({}); o[o.length - 1]['k' + i] = x })
    d.getMap('m').set('nest', { o, list: EDGES.map(x => ({ x, pair: [x, [x]] })) })
    d.getArray('a').push([{ deep: [EDGES] }, EDGES.map(x => ({ x }))])
  }), [['m', MAP], ['a', ARRAY]]))
  out.push(tojsonEntry('Infinity and NaN beside floats', doc(404, d => {
    d.getMap('m').set('inf', Infinity); d.getMap('m').set('half', 0.5); d.getMap('m').set('nan', NaN); d.getMap('m').set('ninf', -Infinity)
    d.getArray('a').push([Infinity, 0.25, NaN])
  }), [['m', MAP], ['a', ARRAY]]))
  out.push(tojsonEntry('integers only (the flag changes nothing)', doc(405, d => {
    d.getMap('m').set('n', 7); d.getMap('m').set('big', 9007199254740992); d.getArray('a').push([1, -2, 1700000000000])
  }), [['m', MAP], ['a', ARRAY], ['t', TEXT]]))
  for (let i = 0; i < SESSIONS; i++) {
    floats(true)
    const s = TJ.randomSession(20240 + 7 * i, true)
    out.push(tojsonEntry('random session ' + s.seed, Buffer.from(s.state, 'hex'), [['m', MAP], ['a', ARRAY], ['t', TEXT]]))
  }
  return out
}

function jsonPart () {
  const out = []
  for (const [note, state] of PJ.edges()) {
    if (note === 'refused: a float attribute' || note === 'refused: a float in a mark' || note === 'refused: a float in an embed') out.push(jsonEntry(note, state))
  }
  out.push(jsonEntry('every edge value as an attribute', doc(411, d => {
    const e = para(frag(d), 0, 'x')
    EDGES.forEach((x, i) => e.setAttribute('v' + i, x))
    e.setAttribute('nest', { o: { list: EDGES.slice(0, 40) } })
  })))
  out.push(jsonEntry('floats in marks, an embed and an attribute of one paragraph', doc(412, d => {
    const e = para(frag(d), 0, null)
    e.setAttribute('lineHeight', 1.5); e.setAttribute('width', 0.5)
    const t = e.get(0)
    t.insert(0, 'sized text', { size: { pt: 10.5 }, opacity: 0.25 })
    t.insertEmbed(5, { image: 'x.png', ratio: 1.3333, at: [103.5, 40.25, -0.000001] }, { size: { pt: 10.5 } })
  })))
  out.push(jsonEntry('an attribute that is not finite (refused with the flag too)', doc(413, d => { para(frag(d), 0, 'x').setAttribute('w', Infinity) })))
  out.push(jsonEntry('a 17-digit float inside an embed, the only float (refused with the flag too)', doc(414, d => {
    para(frag(d), 0, 'ab').get(0).insertEmbed(1, { ratio: 0.1 + 0.2 })
  })))
  out.push(jsonEntry('a float with an exponent inside a mark (refused with the flag too)', doc(415, d => {
    para(frag(d), 0, null).get(0).insert(0, 'tiny', { scale: { v: 1.5e-7 } })
  })))
  out.push(jsonEntry('integers only (the flag changes nothing)', doc(416, d => { para(frag(d), 0, 'x').setAttribute('level', 2) })))
  return out
}

function fieldsPart () {
  const state = doc(421, d => {
    para(d.getXmlFragment('first'), 0, 'plain').setAttribute('level', 1)
    para(d.getXmlFragment('second'), 0, 'floaty').setAttribute('width', 0.5)
    para(d.getXmlFragment('7'), 0, 'index key').setAttribute('x', 103.5)
  })
  return [fieldsEntry('a float in the second field', state, [null, ['first', 'second'], ['first'], ['second', 'first', '7'], ['first', 'no-such-root']])]
}

if (require.main === module) {
  const out = { source: 'tools/floats_corpus.js (yjs 13.5.16 bundle; y-prosemirror restated): node tools/floats_corpus.js tests/golden/floats_v135.json.gz',
    tojson: tojsonPart(), json: jsonPart(), fields: fieldsPart() }
  floats(false)
  fs.writeFileSync(process.argv[2], zlib.gzipSync(Buffer.from(JSON.stringify(out)), { level: 9 }))
  const count = (rows, st, off) => rows.reduce((n, e) => n + e.asks.filter(r => r[r.length - 3] === st && r[r.length - 1] === off).length, 0)
  console.log(JSON.stringify({ tojson: out.tojson.length, json: out.json.length, fields: out.fields.length,
    tojson_ok_was_3: count(out.tojson, 0, 3), json_ok_was_3: count(out.json, 0, 3), fields_ok_was_3: count(out.fields, 0, 3) }))
}
